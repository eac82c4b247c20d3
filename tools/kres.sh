#!/bin/bash
# tools/kres.sh build.log [kernel-name regex]  -> one line per physics kernel (or per kernel matching the regex, e.g. k_swath): VGPRs, spills, scratch, occupancy, LDS (from -Rpass-analysis=kernel-resource-usage output)
python3 - "$1" "${2:-k_physics|k_bd_physics|k_bd_settle}" <<'PY'
import re, sys
cur = None; d = {}
for line in open(sys.argv[1]):
    m = re.search(r'Function Name: (\S+)', line)
    if m: cur = m.group(1); d[cur] = {}; continue
    m = re.search(r'remark: +(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]|TotalSGPRs): (\d+)', line)
    if m and cur: d[cur][m.group(1)] = int(m.group(2))
for k, v in d.items():
    if re.search(sys.argv[2], k):
        print('%-58s' % k[:58], ' '.join('%s=%s' % (a.split(' ')[0], b) for a, b in v.items()))
PY
