// Swath cost of candidate paths over the planner cost maps (bp_swath_cost): compute_swath_cost of the reference's common/swath.py:114-163 -- and with it
// the sums of AStar.get_swath_cost and Path.update -- for K candidates of every env in one launch.  DESIGN.md ("Swath costs") states the semantics.
//
// One wavefront (= one workgroup of 64 threads) per (env, candidate).  The swath is a bit image in LDS, WW = ceil(W / 64) 64-bit words per map row; the
// samples of the path are taken one after the other:
//   1. lanes 0 .. nv-1 transform one footprint vertex each (un-fused: the build has -ffp-contract=off) into s_c / s_r, like k_costmap;
//   2. the pixel box of skimage.draw.polygon is clamped to the map and to the row window IN FLOATING POINT and only then converted to integers;
//   3. the lanes take the pixels of the box, skip those whose bit is already set (consecutive samples overlap almost completely), test the others with
//      pip_arrays (any simple polygon: no convexity is assumed) and set bits with an LDS atomicOr -- a bitwise OR, so the order does not matter.
// Then a lane per row walks the set bits of its row in ascending column order and adds the map's cells, starting from +0.0, and the row sums are added
// in ascending row order, starting from +0.0, by passing them through the lanes in order: the result is a function of the inputs alone (no floating
// atomics).  Rows that no sample's box touched are left out: their row sum is +0.0 and the running total is never -0.0, so adding it changes nothing.
// No global scratch; the mask is written only where the caller asks for it.  Plain vector loads and stores only.
#pragma once
#include "bp_kernels.hpp"

#define BP_SWATH_MAX_WORDS 4096   // H * ceil(W / 64) at most: 32 KB of LDS per workgroup
#define BP_SWATH_HUGE 1e15        // a sample with |x|, |y| or |theta| above this lies off the map as a whole: no sin/cos, no conversion is attempted
// (the outside modes BP_SWATH_CLIP / BP_SWATH_REJECT come from the public header)

struct SwathArgs {
    int H, W, K, P, nv, WW, outside, vec4;   // vec4: the mask rows of every candidate start on a 4-byte boundary and H * W is a multiple of 4
    long long map_stride;                    // doubles between the envs' maps (0: one map for all)
    const double *maps, *paths, *fp;
    const int *lengths, *rows;
    double *costs;
    unsigned char *swaths;
};

__global__ __launch_bounds__(64) void k_swath_cost(const SwathArgs A)
{
    extern __shared__ unsigned long long s_bits[];   // [H][WW]
    __shared__ double s_c[BP_MAXV], s_r[BP_MAXV];
    const int lane = (int)threadIdx.x;
    const size_t cand = blockIdx.x;                  // env * K + candidate
    const size_t env = cand / (size_t)A.K;
    const int H = A.H, W = A.W, WW = A.WW, nv = A.nv;
    for (int i = lane; i < H * WW; i += 64) s_bits[i] = 0ull;
    int len = A.P;
    if (A.lengths) len = min(max(A.lengths[cand], 0), A.P);
    int wlo = 0, whi = H;
    if (A.rows) { wlo = min(max(A.rows[2 * cand], 0), H); whi = min(max(A.rows[2 * cand + 1], 0), H); }
    const double *path = A.paths + cand * (size_t)A.P * 3;
    bool bad = false;                                // a non-finite component in any counted sample: NaN cost, empty mask
    for (int i = lane; i < 3 * len; i += 64) { const double v = path[i]; if (!(__builtin_fabs(v) <= 1.7976931348623157e308)) bad = true; }
    const bool nonfinite = ballot(bad) != 0ull;
    __syncthreads();
    bool outside = false;
    int tlo = H, thi = -1;                           // rows that some sample's box touched
    if (!nonfinite) {
        double fx = 0.0, fy = 0.0;
        if (lane < nv) { fx = A.fp[2 * lane]; fy = A.fp[2 * lane + 1]; }
        for (int i = 0; i < len; i++) {
            const double x = path[3 * i], y = path[3 * i + 1], th = path[3 * i + 2];   // wave-uniform
            if (!(__builtin_fabs(x) <= BP_SWATH_HUGE && __builtin_fabs(y) <= BP_SWATH_HUGE && __builtin_fabs(th) <= BP_SWATH_HUGE)) { outside = true; continue; }
            double sn, cs;
            bp_sincos(th, sn, cs);
            const double vc = x + (cs * fx - sn * fy), vr = y + (sn * fx + cs * fy);
            const bool mine = lane < nv;
            if (mine) { s_c[lane] = vc; s_r[lane] = vr; }
            if (ballot(mine && !(vc >= 0.0 && vc <= (double)(W - 1) && vr >= 0.0 && vr <= (double)(H - 1))) != 0ull) outside = true;
            __syncthreads();
            double rmin = s_r[0], rmax = s_r[0], cmin = s_c[0], cmax = s_c[0];
            for (int j = 1; j < nv; j++) { rmin = fmin(rmin, s_r[j]); rmax = fmax(rmax, s_r[j]); cmin = fmin(cmin, s_c[j]); cmax = fmax(cmax, s_c[j]); }
            // skimage.draw.polygon's box [int(max(0, min)), ceil(max)] clipped to the shape, and the row window: all four bounds end up inside the map
            const double r0 = fmax((double)wlo, __builtin_floor(rmin)), r1 = fmin((double)(whi - 1), __builtin_ceil(rmax));
            const double c0 = fmax(0.0, __builtin_floor(cmin)), c1 = fmin((double)(W - 1), __builtin_ceil(cmax));
            if (r1 >= r0 && c1 >= c0) {
                const int ir0 = (int)r0, ir1 = (int)r1, ic0 = (int)c0, ic1 = (int)c1;
                const int wbox = ic1 - ic0 + 1, npx = (ir1 - ir0 + 1) * wbox;
                for (int q = lane; q < npx; q += 64) {
                    const int rr = q / wbox, ri = ir0 + rr, ci = ic0 + (q - rr * wbox);
                    unsigned long long *const word = &s_bits[ri * WW + (ci >> 6)];
                    const unsigned long long bit = 1ull << (ci & 63);
                    if (*word & bit) continue;
                    if (pip_arrays(s_c, s_r, nv, (double)ci, (double)ri)) atomicOr(word, bit);
                }
                tlo = min(tlo, ir0); thi = max(thi, ir1);
            }
            __syncthreads();   // the next sample overwrites s_c / s_r
        }
    }
    double total = 0.0;
    const bool rejected = A.outside == BP_SWATH_REJECT && outside;
    if (!nonfinite && !rejected) {
        const double *map = A.maps + env * (size_t)A.map_stride;
        for (int base = tlo; base <= thi; base += 64) {
            const int r = base + lane;
            double rs = 0.0;
            if (r <= thi) {
                const double *mrow = map + (size_t)r * W;
                for (int w = 0; w < WW; w++) {
                    unsigned long long bits = s_bits[r * WW + w];
                    while (bits) { rs += mrow[w * 64 + __builtin_ctzll(bits)]; bits &= bits - 1ull; }
                }
            }
            const int n = min(64, thi - base + 1);
            for (int j = 0; j < n; j++) total += __shfl(rs, j);
        }
    }
    if (lane == 0) A.costs[cand] = nonfinite ? __builtin_nan("") : (rejected ? BP_INF : total);
    if (A.swaths) {
        unsigned char *o = A.swaths + cand * (size_t)H * W;
        const int npx = H * W;
        if (A.vec4) {
            for (int p = 4 * lane; p < npx; p += 256) {
                int r = p / W, q = p - r * W;
                unsigned v = 0u;
                for (int b = 0; b < 4; b++) {
                    v |= (unsigned)((s_bits[r * WW + (q >> 6)] >> (q & 63)) & 1ull) << (8 * b);
                    if (++q == W) { q = 0; r++; }
                }
                *(unsigned *)(o + p) = v;
            }
        } else {
            for (int p = lane; p < npx; p += 64) { const int r = p / W, q = p - r * W; o[p] = (unsigned char)((s_bits[r * WW + (q >> 6)] >> (q & 63)) & 1ull); }
        }
    }
}
