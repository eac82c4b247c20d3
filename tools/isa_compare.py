"""Do the kernels of two source trees compile to the same code?  Builds benchpush_amd/csrc/bp_capi.hip of each tree with the library's
flags plus -save-temps (gfx950 device assembly), then compares, for every kernel symbol of the first tree, the metadata fields below and the
instruction count (lines between the kernel's label and its .Lfunc_end that are neither labels, directives nor comments).

    python tools/isa_compare.py <parent tree> <branch tree> [--out report.txt] [--define NAME[=V]]...

--define appends -DNAME[=V] to both builds, so the diagnostic twins (BP_DEBUG_PATHS=1, BP_PROF=1) compare the same way.

Exit status 1 if any kernel of the parent differs or is missing on the branch.  Kernels that exist only on the branch are listed.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

FIELDS = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size", ".kernarg_segment_size"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-std=c++17", "-Wno-unused-value"]


def device_asm(tree, work, defines=()):
    src = os.path.join(os.path.abspath(tree), "benchpush_amd", "csrc", "bp_capi.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-D" + d for d in defines] + ["-save-temps", "-o", os.path.join(work, "lib.so"), src], cwd=work)
    s = [p for p in glob.glob(os.path.join(work, "*.s")) if "gfx950" in p]
    if len(s) != 1:
        raise SystemExit("expected one gfx950 assembly file in %s, found %s" % (work, s))
    return open(s[0]).read()


def kernels(asm):
    """{symbol: {field: value, 'insts': n}} from the amdhsa metadata and the function bodies."""
    out = {}
    meta = asm[asm.find("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"\n\s+\.symbol:\s+(\S+)", "\n" + blk)
        if not m:
            continue
        sym = m.group(1)
        name = sym[:-3] if sym.endswith(".kd") else sym
        d = {}
        for f in FIELDS:
            fm = re.search(r"\n\s+" + re.escape(f) + r":\s+(\S+)", "\n" + blk)
            d[f] = fm.group(1) if fm else None
        out[name] = d
    lines = asm.split("\n")
    for name, d in out.items():
        start = next((i for i, ln in enumerate(lines) if ln.split(";")[0].strip() == name + ":"), None)
        if start is None:
            d["insts"] = None
            continue
        n = 0
        for ln in lines[start + 1:]:
            t = ln.strip()
            if t.startswith(".Lfunc_end"):
                break
            if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
                continue
            n += 1
        d["insts"] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--out")
    ap.add_argument("--define", action="append", default=[], metavar="NAME[=V]")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as w0, tempfile.TemporaryDirectory() as w1:
        k0, k1 = kernels(device_asm(a.parent, w0, a.define)), kernels(device_asm(a.branch, w1, a.define))
    rows, bad = [], 0
    keys = FIELDS + ["insts"]
    for name in sorted(k0):
        if name not in k1:
            rows.append("MISSING  %s" % name)
            bad += 1
            continue
        diff = [k for k in keys if k0[name][k] != k1[name][k]]
        short = " ".join("%s=%s" % (k.lstrip(".").replace("_count", "").replace("_segment_fixed_size", ""), k0[name][k]) for k in keys)
        if diff:
            bad += 1
            rows.append("DIFFERS  %s  %s" % (name, "; ".join("%s %s -> %s" % (k, k0[name][k], k1[name][k]) for k in diff)))
        else:
            rows.append("same     %s  %s" % (name, short))
    for name in sorted(set(k1) - set(k0)):
        rows.append("new      %s  %s" % (name, " ".join("%s=%s" % (k.lstrip("."), k1[name][k]) for k in keys)))
    rows.append("%d kernels of the parent, %d differ or are missing" % (len(k0), bad))
    text = "\n".join(rows)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
