// State records: save / restore / clone of whole environments between steps (bp_save_state, bp_load_state, bp_clone_state).
//
// Between two bp_step calls an env lives entirely in the persistent per-env arrays of DevPtrs / BdPtrs.  A state record is a fixed-size byte image of
// the arrays that a later API call on that env can depend on, one 16-byte aligned segment per array behind a 32-byte header:
//   [BpStateHeader][segment 1, padded to 16 bytes][segment 2] ...
// ONE host-side table (bp_state_layout below) lists the arrays; the three kernels walk it, so an array is either in the record or not in exactly one place.
// Whoever adds a per-env array to DevPtrs / BdPtrs registers it there (or says in its comment why a record does not need it).
#pragma once
#include "bp_boxdelivery.hpp"

#define BP_STATE_MAGIC 0x3130534D41504221ull   // "!BPAMS01", little endian
#define BP_STATE_HDR 32                        // bytes of BpStateHeader
#define BP_STATE_MAXSEG 64
#define BP_STATE_THREADS 256
enum { BP_SEG_COPY = 0, BP_SEG_OR32 = 1, BP_SEG_HEADER = 2 };

struct BpStateHeader {
    unsigned long long magic, bytes, layout_id, reserved;
};
static_assert(sizeof(BpStateHeader) == BP_STATE_HDR, "record header");

// One row of the segment table (the same struct on the host and in device memory).
struct BpStateSeg {
    unsigned char *base;       // first env's slot of the array (null in the pure layout query)
    unsigned long long span;   // bytes per env slot
    unsigned long long off;    // byte offset of the segment in the record, a multiple of 16
    unsigned width;            // widest access (bytes, power of two <= 16) that base + env * span is aligned for with every env
    unsigned kind;             // BP_SEG_COPY; BP_SEG_OR32: one int32 whose saved bits are OR-ed into the destination (e_err); BP_SEG_HEADER
};
struct BpStateLayout {
    int nseg = 0;
    unsigned long long bytes = 0;   // bytes of one record (a multiple of 16)
    BpStateSeg seg[BP_STATE_MAXSEG];
    const char *name[BP_STATE_MAXSEG];
};

inline void bp_state_add(BpStateLayout &L, const char *name, const void *base, unsigned long long span, unsigned kind = BP_SEG_COPY)
{
    if (L.nseg >= BP_STATE_MAXSEG) return;   // (static table below: 50 rows at most; bp_state_layout's callers check nseg)
    BpStateSeg &s = L.seg[L.nseg];
    s.base = (unsigned char *)const_cast<void *>(base);
    s.span = span;
    s.off = L.bytes;
    unsigned w = 16;
    while (w > 1 && (span % w) != 0) w >>= 1;    // every array starts on a hipMalloc boundary (256 bytes): the span alone decides
    s.width = w;
    s.kind = kind;
    L.name[L.nseg] = name;
    L.nseg++;
    L.bytes += (span + 15ull) & ~15ull;
}

// THE table.  D / Q may be zeroed (pure layout query: only spans and offsets are used); box = box-delivery / area-clearing handle; map_cells = SH * SW of its
// small-map window.  What is left out and why is stated at the members of DevPtrs / BdPtrs and in DESIGN.md ("State records").
inline BpStateLayout bp_state_layout(const DevPtrs &D, const BdPtrs &Q, int nbcap, bool box, int map_cells)
{
    BpStateLayout L;
    bp_state_add(L, "header", nullptr, BP_STATE_HDR, BP_SEG_HEADER);
    const unsigned long long nb = (unsigned long long)nbcap;
#define BP_SEG_D(arr, elems) bp_state_add(L, #arr, D.arr, sizeof(*D.arr) * (unsigned long long)(elems))
#define BP_SEG_Q(arr, elems) bp_state_add(L, #arr, Q.arr, sizeof(*Q.arr) * (unsigned long long)(elems))
    // body state
    BP_SEG_D(pxy, nb); BP_SEG_D(ang, nb); BP_SEG_D(rot, nb); BP_SEG_D(velv, nb); BP_SEG_D(velw, nb); BP_SEG_D(velb, nb);
    BP_SEG_D(wv, nb * BP_MAXV); BP_SEG_D(wn, nb * BP_MAXV); BP_SEG_D(pv, nb * BP_MAXV);
    BP_SEG_D(bb, nb); BP_SEG_D(fat, nb);
    BP_SEG_D(adj, nb * BP_KADJ); BP_SEG_D(adjn, nb); BP_SEG_D(hint, nb * BP_KADJ);
    // the 64 arbiter slots
    BP_SEG_D(a_key, BP_ACAP); BP_SEG_D(a_stamp, BP_ACAP); BP_SEG_D(a_sc, BP_ACAP); BP_SEG_D(a_h0, BP_ACAP); BP_SEG_D(a_h1, BP_ACAP);
    BP_SEG_D(a_d, BP_ACAP * 14);
    // scalars
    BP_SEG_D(e_trial, 1); BP_SEG_D(e_episode, 1); BP_SEG_D(e_nb, 1);
    bp_state_add(L, "e_err", D.e_err, sizeof(int), BP_SEG_OR32);
    BP_SEG_D(e_flags, 1); BP_SEG_D(e_prevdist, 1); BP_SEG_D(e_stamp, 1); BP_SEG_D(e_currdt, 1); BP_SEG_D(e_total_work, 1);
    BP_SEG_D(e_ke, 1); BP_SEG_D(e_imp, 1); BP_SEG_D(e_cnt, 4);
    // last step and episode metrics
    BP_SEG_D(e_lastrew, 1); BP_SEG_D(e_lastflag, 1);
    BP_SEG_D(m_acc, 8); BP_SEG_D(m_rows, BP_EPM_COUNT); BP_SEG_D(m_ring, BP_EPM_RING * BP_EPM_COUNT); BP_SEG_D(m_sum, BP_EPM_COUNT);
    BP_SEG_D(m_count, 1); BP_SEG_D(m_open, 1);
    if (box) {
        BP_SEG_Q(alive, BD_MAXBOX); BP_SEG_Q(order, BD_MAXBOX); BP_SEG_Q(nalive, 1); BP_SEG_Q(nprev, 1);
        BP_SEG_Q(boxdist, BD_MAXBOX); BP_SEG_Q(boxpos, BD_MAXBOX); BP_SEG_Q(prev, BD_MAXBOX * 4);
        BP_SEG_Q(cum, 4); BP_SEG_Q(cnt, 4); BP_SEG_Q(wp, BD_MAXWP * 3); BP_SEG_Q(nwp, 1); BP_SEG_Q(stepf, 8);
        BP_SEG_Q(cleared, BD_MAXBOX); BP_SEG_Q(m_box, BD_MAXBOX * 3);
        BP_SEG_Q(rmap, map_cells);   // observation channel 2 is read from it: bp_observe straight after a load must give the saved observation
    }
#undef BP_SEG_D
#undef BP_SEG_Q
    return L;
}

// The part of the layout id that the shapes alone decide (bp_state_layout_query); a handle hashes its configuration and scenario tables on top.
inline unsigned long long bp_state_structure_id(const BpStateLayout &L, int env_kind, int task, int nbcap, int map_cells)
{
    unsigned long long h = bp_fnv1a_i64(BP_STATE_MAGIC, 0xCBF29CE484222325ull);
    const long long v[] = {env_kind, task, nbcap, BP_MAXV, BP_KADJ, BP_ACAP, BD_MAXBOX, BD_MAXWP, map_cells, L.nseg, (long long)L.bytes};
    h = bp_fnv1a(v, sizeof(v), h);
    for (int i = 0; i < L.nseg; i++) { h = bp_fnv1a_i64((long long)L.seg[i].span, h); h = bp_fnv1a_i64((long long)L.seg[i].off, h); }
    return h;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------------
// A record is cut into 16-byte slots; thread t of a workgroup handles slot (tile * U + u) * 256 + t for u = 0 .. U - 1: consecutive lanes touch consecutive
// addresses on both sides, the record side is always one 16-byte access, the env side takes 16 / width accesses of the segment's width (most segments: one).
// A record is split over ceil(slots / (256 * U)) workgroups, so a fan-out of one env to 16 still fills the device.  The segment of a slot is found by a
// binary search over the table's first slots in LDS (6 probes; the copy is bound by HBM, not by these).  Plain vector loads and stores only.
__device__ __forceinline__ uint4 state_ld(const unsigned char *__restrict__ p, const unsigned w, const unsigned n)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (w == 16) v = *(const uint4 *)p;
    else if (w == 8) {
        const uint2 a = *(const uint2 *)p; v.x = a.x; v.y = a.y;
        if (n > 8) { const uint2 b = *(const uint2 *)(p + 8); v.z = b.x; v.w = b.y; }
    } else if (w == 4) {
        const unsigned *q = (const unsigned *)p;
        v.x = q[0];
        if (n > 4) v.y = q[1];
        if (n > 8) v.z = q[2];
        if (n > 12) v.w = q[3];
    } else {
        unsigned r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; i++) if ((unsigned)i < n) r[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
        v = make_uint4(r[0], r[1], r[2], r[3]);
    }
    return v;
}
__device__ __forceinline__ void state_st(unsigned char *__restrict__ p, const unsigned w, const unsigned n, const uint4 v)
{
    if (w == 16) *(uint4 *)p = v;
    else if (w == 8) {
        *(uint2 *)p = make_uint2(v.x, v.y);
        if (n > 8) *(uint2 *)(p + 8) = make_uint2(v.z, v.w);
    } else if (w == 4) {
        unsigned *q = (unsigned *)p;
        q[0] = v.x;
        if (n > 4) q[1] = v.y;
        if (n > 8) q[2] = v.z;
        if (n > 12) q[3] = v.w;
    } else {
        const unsigned r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; i++) if ((unsigned)i < n) p[i] = (unsigned char)(r[i >> 2] >> (8 * (i & 3)));
    }
}

struct StateArgs {
    const BpStateSeg *table;   // device copy of the handle's table
    int nseg;
    unsigned nslots;           // record bytes / 16
    unsigned tiles;            // workgroups per record
    int rec0;                  // first record of this launch (launches are chunked below 2^31 workgroups)
    const int *ids_a;          // pack: source envs; unpack: destination envs; clone: source envs
    const int *ids_b;          // clone: destination envs
    unsigned char *records;    // pack: written; unpack: read
    BpStateHeader hdr;
};
enum { STATE_PACK = 0, STATE_UNPACK = 1, STATE_CLONE = 2 };

template <int MODE, int U>
__device__ __forceinline__ void state_body(const StateArgs &A)
{
    __shared__ BpStateSeg s_seg[BP_STATE_MAXSEG];
    __shared__ unsigned s_first[BP_STATE_MAXSEG + 1];
    const unsigned tid = threadIdx.x;
    if (tid < (unsigned)A.nseg) { const BpStateSeg s = A.table[tid]; s_seg[tid] = s; s_first[tid] = (unsigned)(s.off >> 4); }
    if (tid == 0) s_first[A.nseg] = A.nslots;
    __syncthreads();
    const unsigned rec = (unsigned)A.rec0 + blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
    const unsigned long long ea = (unsigned long long)A.ids_a[rec];
    const unsigned long long eb = MODE == STATE_CLONE ? (unsigned long long)A.ids_b[rec] : 0ull;
    unsigned char *const record = MODE == STATE_CLONE ? nullptr : A.records + (unsigned long long)rec * ((unsigned long long)A.nslots << 4);
    // the segment of each of this thread's slots
    int seg[U];
    bool fast = true;   // wave-uniform: every slot of the wave lies in one 16-byte-wide plain segment per u -- nearly every tile of a record
#pragma unroll
    for (int u = 0; u < U; u++) {
        const unsigned slot = (tile * U + u) * BP_STATE_THREADS + tid;
        int lo = 0, hi = A.nseg;            // largest lo with s_first[lo] <= slot
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_first[mid] <= slot) lo = mid; else hi = mid; }
        seg[u] = lo;
        const bool ok = slot < A.nslots && lo == __builtin_amdgcn_readfirstlane(lo) && s_seg[lo].width == 16u && s_seg[lo].kind == BP_SEG_COPY;
        fast = fast && __all(ok);
    }
    if (fast) {
        // straight-line copy: U loads in flight per lane, then U stores
        uint4 val[U];
        unsigned char *dst[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned slot = (tile * U + u) * BP_STATE_THREADS + tid;
            const int sg = __builtin_amdgcn_readfirstlane(seg[u]);
            const BpStateSeg S = s_seg[sg];
            const unsigned long long in = (unsigned long long)(slot - s_first[sg]) << 4;
            const unsigned char *src = MODE == STATE_UNPACK ? record + ((unsigned long long)slot << 4) : S.base + ea * S.span + in;
            dst[u] = MODE == STATE_PACK ? record + ((unsigned long long)slot << 4) : S.base + (MODE == STATE_CLONE ? eb : ea) * S.span + in;
            val[u] = *(const uint4 *)src;
        }
#pragma unroll
        for (int u = 0; u < U; u++) *(uint4 *)dst[u] = val[u];
        return;
    }
    // general path: header, narrow segments, segment boundaries inside the wave, the tail of the record
    for (int u = 0; u < U; u++) {
        const unsigned slot = (tile * U + u) * BP_STATE_THREADS + tid;
        if (slot >= A.nslots) continue;
        const int lo = seg[u];
        const BpStateSeg S = s_seg[lo];
        const unsigned long long in = (unsigned long long)(slot - s_first[lo]) << 4;   // byte offset inside the segment
        if (in >= S.span) continue;          // (cannot happen: a segment's padding is below 16 bytes)
        const unsigned n = (unsigned)(S.span - in < 16ull ? S.span - in : 16ull);
        unsigned char *const rslot = MODE == STATE_CLONE ? nullptr : record + ((unsigned long long)slot << 4);
        if (S.kind == BP_SEG_HEADER) {
            if (MODE == STATE_PACK)
                *(uint4 *)rslot = in == 0 ? make_uint4((unsigned)A.hdr.magic, (unsigned)(A.hdr.magic >> 32), (unsigned)A.hdr.bytes, (unsigned)(A.hdr.bytes >> 32))
                                          : make_uint4((unsigned)A.hdr.layout_id, (unsigned)(A.hdr.layout_id >> 32), 0u, 0u);
            continue;
        }
        // pack writes a record's padding too (zeros): records of equal states are equal bytes
        const uint4 v = MODE == STATE_UNPACK ? *(const uint4 *)rslot : state_ld(S.base + ea * S.span + in, S.width, n);
        if (MODE == STATE_PACK) { *(uint4 *)rslot = v; continue; }
        unsigned char *const d = S.base + (MODE == STATE_CLONE ? eb : ea) * S.span + in;
        if (S.kind == BP_SEG_OR32) { if (v.x) atomicOr((int *)d, (int)v.x); }
        else state_st(d, S.width, n, v);
    }
}
template <int U> __global__ __launch_bounds__(BP_STATE_THREADS) void k_state_pack(const StateArgs A) { state_body<STATE_PACK, U>(A); }
template <int U> __global__ __launch_bounds__(BP_STATE_THREADS) void k_state_unpack(const StateArgs A) { state_body<STATE_UNPACK, U>(A); }
template <int U> __global__ __launch_bounds__(BP_STATE_THREADS) void k_state_clone(const StateArgs A) { state_body<STATE_CLONE, U>(A); }
