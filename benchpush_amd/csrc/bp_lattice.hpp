// Batched lattice A* over the planner cost maps (bp_lattice_search): AStar.search of the reference's a_star_search.py for the high-level planner
// (goal_pos = None, occ_map = None, smoothing off), one search per env in one launch.  DESIGN.md ("Lattice search") states the semantics and
// tests/lattice_ref.py restates them in numpy + heapq; this kernel is held to that restatement with ==.
//
// One wavefront (= one workgroup of 64 threads) per env.  The search is sequential -- pop, expand, relax, push -- and every lane runs it with the same
// (wave-uniform) values: each lane reads back only what it stored itself, so no fence or barrier is needed between a store and a later load of the same
// address.  The parallel part is the swath cost of an edge: lane r holds row r of the S x S bit mask of the edge (S <= 64, the documented limit), walks
// its set bits in ascending column order adding the map's cells from +0.0, and the row sums are added in ascending row order from +0.0 by passing them
// through the lanes -- the convention of k_swath_cost; no floating atomics, the result is a function of the inputs alone.
//
// Where things live.  LDS: nothing -- the primitive tables (at most 4 x 32 edges) travel in the kernel argument block and end up in scalar registers /
// the constant cache, and a wave needs no staging area of its own, so the occupancy is bounded by registers alone and the other waves of the CU hide the
// latency of the sequential part.  Global memory, in the caller's workspace, per env: the hash index (open addressing, linear probing, a power of two of
// at least 2 * node_capacity words, node id + 1 or 0), the node records (24 bytes: g, key, parent, edge, closed) and the binary heap (16 bytes per entry:
// f, key, node id; stale entries are skipped at pop because their node is closed or, while open, sorts behind its current entry).  The masks are an
// input; the kernel rasterises nothing.  Every loop is bounded by a cap: pops by the pushes (at most 32 per expansion, expansions <= max_expansions),
// probes by the index size, sift loops by the heap size, the back-walk by the node count.  Plain vector loads and stores only.
#pragma once
#include "bp_device.hpp"

#define BP_LAT_MAX_EDGES 32     // per base heading
#define BP_LAT_MAX_BASE 4       // nh = 16 -> 4 base headings
#define BP_LAT_KEY_OFF 4096     // |i|, |j| < 4096 sub-units: key = (j + 4096) << 18 | (i + 4096) << 5 | h
#define BP_LAT_COORD_MAX 1e9    // a start / goal beyond this, or not finite, has no path (no conversion to int is attempted)
#define BP_LAT_TWO_PI 6.283185307179586

struct LatNode { double g; unsigned key; int parent, edge, closed; };             // 24 bytes
struct __attribute__((aligned(16))) LatEntry { double f; unsigned key, id; };     // 16 bytes

struct LatticeArgs {
    int H, W, S, mv, nh, nb, ne_max, margin, h_baseline, max_exp, ncap, hcap, qcap, nmax;
    long long map_stride, mask_stride;      // doubles / 64-bit words between the envs (0: shared)
    unsigned long long ws_stride, off_nodes, off_heap;   // bytes
    double u, weight, r;
    const double *maps, *starts, *goal_y;
    const unsigned char *active;
    const unsigned long long *masks;
    unsigned char *ws;
    int *status, *expanded, *n_nodes, *edges;
    double *g, *nodes;
    int ne[BP_LAT_MAX_BASE];
    short ex[BP_LAT_MAX_BASE * BP_LAT_MAX_EDGES], ey[BP_LAT_MAX_BASE * BP_LAT_MAX_EDGES];
    signed char eh[BP_LAT_MAX_BASE * BP_LAT_MAX_EDGES];
    double len[BP_LAT_MAX_BASE * BP_LAT_MAX_EDGES];
};

// fdlibm's e_acos.c, operation by operation (un-fused; IEEE division and square root).  tests/lattice_ref.py: bp_acos is the same in pure Python.
__device__ __forceinline__ double bp_acos_pq(const double z)
{
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
    const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    return p / q;
}
__device__ __forceinline__ double bp_acos(const double x)
{
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const unsigned hx = (unsigned)__double2hiint(x), lx = (unsigned)__double2loint(x), ix = hx & 0x7fffffffu;
    if (ix >= 0x3ff00000u) {
        if (((ix - 0x3ff00000u) | lx) == 0u) return hx < 0x80000000u ? 0.0 : pi + 2.0 * pio2_lo;
        return __builtin_nan("");
    }
    if (ix < 0x3fe00000u) {
        if (ix <= 0x3c600000u) return pio2_hi + pio2_lo;
        const double r = bp_acos_pq(x * x);
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (hx >= 0x80000000u) {
        const double z = (1.0 + x) * 0.5, s = __dsqrt_rn(z);
        const double w = bp_acos_pq(z) * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5, s = __dsqrt_rn(z);
    const double df = __hiloint2double(__double2hiint(s), 0);
    const double c = (z - df * df) / (s + df);
    const double w = bp_acos_pq(z) * s + c;
    return 2.0 * (df + w);
}

// dubins_heuristic(q, goal, r_min, (b0, b1))[0] of the reference's common/dubins_helpers/heuristic.py
__device__ __forceinline__ double lat_dubins_h(const double x, const double y, const double th, const double goal, const double r, const double b0, const double b1)
{
    if (y >= goal) return 0.0;
    const double hpi = BP_PI / 2, pi3 = 3 * BP_PI / 2, pi5 = 5 * BP_PI / 2;
    double s, c;
    bp_sincos(th, s, c);
    const double m = (th <= hpi || th >= pi3) ? 1.0 : -1.0;
    const double mr = m * r;
    double omega_y = y + mr * c;
    double h, xx;
    if (omega_y >= goal) {
        const double n = th <= hpi ? 0.0 : (th <= pi3 ? BP_PI : 2 * BP_PI);
        const double d = omega_y - goal;
        const double theta = m * bp_acos(d / r) + n;
        h = r * __builtin_fabs(th - theta);
        const double rad = r * r - d * d;
        xx = (x - mr * s) + m * (rad >= 0.0 ? __dsqrt_rn(rad) : __builtin_nan(""));
    } else {
        h = (r * fmin(__builtin_fabs(hpi - th), __builtin_fabs(pi5 - th)) + goal) - omega_y;
        xx = mr * (1.0 - s) + x;
    }
    if (b0 > xx || xx > b1) {
        if (0.0 <= th && th <= BP_PI) h = BP_INF;
        else {
            omega_y = y - (omega_y - y);
            const double omega_x = x + mr * s;
            if (b0 > omega_x || omega_x > b1) h = BP_INF;
            else {
                h = (r * fmax(__builtin_fabs(hpi - th), __builtin_fabs(pi5 - th)) + goal) - omega_y;
                xx = (-m) * r * (1.0 - s) + x;
                if (b0 > xx || xx > b1) h = BP_INF;
            }
        }
    }
    return h;
}

__device__ __forceinline__ bool lat_less(const LatEntry &a, const LatEntry &b) { return a.f < b.f || (a.f == b.f && a.key < b.key); }

__global__ __launch_bounds__(64) void k_lattice_search(const LatticeArgs A)
{
    const int lane = (int)threadIdx.x;
    const size_t env = blockIdx.x;
    if (A.active && !A.active[env]) { if (lane == 0) A.status[env] = BP_LATTICE_SKIPPED; return; }
    unsigned char *const ws = A.ws + env * A.ws_stride;
    unsigned *const hidx = (unsigned *)ws;
    LatNode *const nodes = (LatNode *)(ws + A.off_nodes);
    LatEntry *const heap = (LatEntry *)(ws + A.off_heap);
    const int H = A.H, W = A.W, mv = A.mv, nb = A.nb, nh = A.nh;
    const unsigned hmask = (unsigned)A.hcap - 1u;
    for (int i = lane; i < A.hcap; i += 64) hidx[i] = 0u;
    __syncthreads();   // the index is cleared by all lanes, then read by each of them

    const double x0 = A.starts[3 * env], y0 = A.starts[3 * env + 1], th0 = A.starts[3 * env + 2], goal_y = A.goal_y[env];
    int status = BP_LATTICE_NO_PATH, expanded = 0, n_out = 0;
    double g_goal = BP_INF;
    const bool ok = __builtin_fabs(x0) <= BP_LAT_COORD_MAX && __builtin_fabs(y0) <= BP_LAT_COORD_MAX && __builtin_fabs(th0) <= BP_LAT_COORD_MAX &&
                    __builtin_fabs(goal_y) <= BP_LAT_COORD_MAX && x0 >= 0.0 && x0 <= (double)W && y0 >= 0.0 && y0 <= (double)H;
    if (ok) {
        double th0m = fmod(th0, BP_LAT_TWO_PI);           // Python's %: the sign of the divisor
        if (th0m != 0.0) { if (th0m < 0.0) th0m += BP_LAT_TWO_PI; } else th0m = 0.0;
        double s0, c0;
        bp_sincos(th0m, s0, c0);
        const double u = A.u, spacing = BP_LAT_TWO_PI / (double)nh, Wd = (double)W, Hd = (double)H;
        const int lo = max(0, (int)y0 - A.margin), hi = min(H, (int)goal_y + A.margin);
        const double *const map = A.maps + env * (size_t)A.map_stride;
        const unsigned long long *const masks = A.masks + env * (size_t)A.mask_stride;

#define LAT_POS(i_, j_, X_, Y_) { const double a_ = (double)(i_) * u, b_ = (double)(j_) * u; X_ = x0 + (c0 * a_ - s0 * b_); Y_ = y0 + (s0 * a_ + c0 * b_); }
#define LAT_WORLD_H(h_, t_) { t_ = (double)(h_) * spacing + th0m; if (t_ >= BP_LAT_TWO_PI) t_ -= BP_LAT_TWO_PI; }
        auto fscore = [&](const double g, const double X, const double Y, const int h) -> double {
            if (A.weight == 0.0) return g;
            double hv;
            if (A.h_baseline) hv = fmax(0.0, goal_y - Y);
            else { double t; LAT_WORLD_H(h, t); hv = lat_dubins_h(X, Y, t, goal_y, A.r, 0.0, Wd); }
            const double f = g + A.weight * hv;
            return f == f ? f : BP_INF;
        };

        // the start node: id 0
        const unsigned key0 = ((unsigned)BP_LAT_KEY_OFF << 18) | ((unsigned)BP_LAT_KEY_OFF << 5);
        int n_nodes = 1, n_heap = 1;
        { LatNode s; s.g = 0.0; s.key = key0; s.parent = -1; s.edge = -1; s.closed = 0; nodes[0] = s; }
        hidx[(key0 * 2654435761u) & hmask] = 1u;
        { LatEntry e; e.f = fscore(0.0, x0, y0, 0); e.key = key0; e.id = 0u; heap[0] = e; }
        int goal = -1;
        bool capped = false;
        while (n_heap > 0 && !capped) {
            // pop
            const LatEntry top = heap[0];
            const LatEntry last = heap[--n_heap];
            for (int i = 0;;) {
                int c = 2 * i + 1;
                if (c >= n_heap) { if (n_heap > 0) heap[i] = last; break; }
                LatEntry ce = heap[c];
                if (c + 1 < n_heap) { const LatEntry c2 = heap[c + 1]; if (lat_less(c2, ce)) { ce = c2; c++; } }
                if (lat_less(ce, last)) { heap[i] = ce; i = c; } else { heap[i] = last; break; }
            }
            const int cur = (int)top.id;
            const LatNode nd = nodes[cur];
            if (nd.closed) continue;
            const int h = (int)(nd.key & 31u), i = (int)((nd.key >> 5) & 8191u) - BP_LAT_KEY_OFF, j = (int)(nd.key >> 18) - BP_LAT_KEY_OFF;
            double X, Y;
            LAT_POS(i, j, X, Y);
            if (Y >= goal_y) { goal = cur; break; }
            if (expanded >= A.max_exp) { capped = true; break; }
            nodes[cur].closed = 1;
            expanded++;
            const int b = h % nb, q = h / nb;
            const int ix = (int)X, iy = (int)Y;
            const int ne = A.ne[b];
            for (int k = 0; k < ne; k++) {
                const int t = b * BP_LAT_MAX_EDGES + k;
                const int ex = A.ex[t], ey = A.ey[t];
                const int rx = q == 0 ? ex : (q == 1 ? -ey : (q == 2 ? -ex : ey)), ry = q == 0 ? ey : (q == 1 ? ex : (q == 2 ? -ey : -ex));
                const int i2 = i + rx, j2 = j + ry, h2 = (q * nb + (int)A.eh[t]) % nh;
                double X2, Y2;
                LAT_POS(i2, j2, X2, Y2);
                if (!(0.0 < X2 && X2 < Wd && 0.0 < Y2 && Y2 < Hd)) continue;
                // an accepted position lies on the map, and the host has checked that the map's diagonal fits the key
                const unsigned key2 = ((unsigned)(j2 + BP_LAT_KEY_OFF) << 18) | ((unsigned)(i2 + BP_LAT_KEY_OFF) << 5) | (unsigned)h2;
                unsigned slot = (key2 * 2654435761u) & hmask;
                int id2 = -1;
                for (int p = 0; p < A.hcap; p++) {
                    const unsigned v = hidx[slot];
                    if (v == 0u) break;
                    if (nodes[v - 1u].key == key2) { id2 = (int)(v - 1u); break; }
                    slot = (slot + 1u) & hmask;
                }
                double g2 = BP_INF;
                if (id2 >= 0) { const LatNode n2 = nodes[id2]; if (n2.closed) continue; g2 = n2.g; }
                // swath cost of the edge: lane = mask row
                unsigned long long word = 0ull;
                if (lane < A.S) word = masks[(size_t)(h * A.ne_max + k) * A.S + lane];
                const int row = iy + lane - mv, c0col = ix - mv;
                bool bad = false;
                double rs = 0.0;
                if (word) {
                    const int cmin = c0col + __builtin_ctzll(word), cmax = c0col + 63 - __builtin_clzll(word);
                    if (row < lo || row >= hi || cmin < 0 || cmax >= W) bad = true;
                    else {
                        const double *const mrow = map + (size_t)row * W + c0col;
                        unsigned long long bits = word;
                        while (bits) { rs += mrow[__builtin_ctzll(bits)]; bits &= bits - 1ull; }
                    }
                }
                double sw = 0.0;
                if (ballot(bad) != 0ull) sw = BP_INF;
                else {
                    unsigned long long rows = ballot(word != 0ull);
                    while (rows) { sw += __shfl(rs, __builtin_ctzll(rows)); rows &= rows - 1ull; }
                }
                const double tg = (nd.g + sw) + A.len[t];
                if (!(tg < g2)) continue;
                if (id2 < 0) {
                    if (n_nodes >= A.ncap) { capped = true; break; }
                    if (n_heap >= A.qcap) { capped = true; break; }
                    id2 = n_nodes++;
                    hidx[slot] = (unsigned)id2 + 1u;
                } else if (n_heap >= A.qcap) { capped = true; break; }
                { LatNode n2; n2.g = tg; n2.key = key2; n2.parent = cur; n2.edge = b * A.ne_max + k; n2.closed = 0; nodes[id2] = n2; }
                // push
                LatEntry e; e.f = fscore(tg, X2, Y2, h2); e.key = key2; e.id = (unsigned)id2;
                int p = n_heap++;
                while (p > 0) {
                    const int par = (p - 1) >> 1;
                    const LatEntry pe = heap[par];
                    if (lat_less(e, pe)) { heap[p] = pe; p = par; } else break;
                }
                heap[p] = e;
            }
        }
        if (capped) status = BP_LATTICE_CAP;
        else if (goal > 0) {
            int n = 0;
            for (int c = goal; c >= 0 && n <= n_nodes; c = nodes[c].parent) n++;
            if (n > A.nmax) status = BP_LATTICE_CAP;
            else {
                status = BP_LATTICE_FOUND; n_out = n; g_goal = nodes[goal].g;
                double *const on = A.nodes + env * (size_t)A.nmax * 3;
                int *const oe = A.edges + env * (size_t)A.nmax;
                int c = goal;
                for (int p = n - 1; p >= 0 && c >= 0; p--) {
                    const LatNode nd = nodes[c];
                    const int h = (int)(nd.key & 31u), i = (int)((nd.key >> 5) & 8191u) - BP_LAT_KEY_OFF, j = (int)(nd.key >> 18) - BP_LAT_KEY_OFF;
                    double X, Y, t;
                    LAT_POS(i, j, X, Y);
                    LAT_WORLD_H(h, t);
                    if (lane == 0) { on[3 * p] = X; on[3 * p + 1] = Y; on[3 * p + 2] = t; oe[p] = nd.edge; }
                    c = nd.parent;
                }
            }
        }
#undef LAT_POS
#undef LAT_WORLD_H
    }
    if (lane == 0) { A.status[env] = status; A.g[env] = g_goal; A.expanded[env] = expanded; A.n_nodes[env] = n_out; }
}
