// k_render: rgb_array frames of the four tasks (benchpush_amd/render.py states the frame; include/benchpush_amd.h the ABI).
//
// One workgroup per (frame, 64 x 16 pixel tile), four pixels per thread.  The frame's items -- layer-0 primitives, the shape slots in the
// trial's draw order, the env's path segments, layer-1 primitives -- are walked from the top of the draw order down in passes of
// RENDER_THREADS candidates: each pass culls its candidates against the tile by pixel bounding box, compacts the survivors in draw order
// into LDS (wave ballots), stages their pixel-space vertices there, and every pixel that no higher item has claimed takes the colour of the
// first survivor that covers it.  A pixel's colour is therefore a function of the frame definition alone; each output byte has one writer.
// The kernel reads handle state (world vertices, counts, trial, body count, box liveness) and never writes it.
#pragma once
#include "bp_boxdelivery.hpp"

#define RENDER_THREADS 256
#define RENDER_TW 64             // tile width in pixels: 16 threads x 4 pixels
#define RENDER_TH 16             // tile height: one row per 16 threads
#define RENDER_VCAP 2048         // staged vertices per pass; items beyond are read from global memory per test
#define RENDER_MARGIN 1e-6       // bounding boxes are widened by this (pip_arrays accepts points within 1e-12 of a vertex)

struct RenderK {
    // handle state (read only)
    const d2 *wv;               // [E][nbcap][MAXV] world vertices
    const int *sc_nv;           // [T][nbcap]
    const double4 *sc_prop;     // [T][nbcap] shape radius in .x
    const int *e_trial, *e_nb;  // [E]
    const unsigned char *alive; // box-delivery / area-clearing: [E][BD_MAXBOX] box k of slot first_box + k is in the space; null otherwise
    int first_box, nbox, nbcap, num_envs, num_trials;
    // draw table
    const int *order;           // [T][nslot] slots bottom first, -1 = none
    const unsigned *rgb;        // [T][nslot]
    const bp_render_prim *prims;// [nunder + nover], layer 0 first
    int nslot, nunder, nover;
    // call
    const int *env_ids;         // [k]
    const double *paths;        // [k][max_path][2] or null
    const int *path_len;        // [k] or null
    int max_path, width, height, tiles_x, tiles;
    double scale, tx, ty, cx, cy, path_half;
    unsigned background;
    unsigned char *out;         // [k][H][W][3]
    int frame0;                 // first frame of this launch (frames are launched in chunks)
};

// candidate j of frame f: kind (0 polygon, 1 capsule, -1 nothing), its vertex count, colour and capsule half-width; vertices via render_vert
struct RItem {
    int kind, nv;
    unsigned rgb;
    double h;
    int src, idx;    // src 0: slot idx, 1: primitive idx, 2: path segment idx
};

__device__ __forceinline__ RItem render_item(const RenderK &K, int env, int trial, int plen, int j)
{
    RItem it; it.kind = -1; it.nv = 0; it.rgb = 0; it.h = 0.0; it.src = 0; it.idx = 0;
    const int nseg = plen >= 2 ? plen - 1 : 0;
    int p = -1;
    if (j < K.nunder) p = j;
    else if (j < K.nunder + K.nslot) {
        const int q = j - K.nunder;
        const int s = K.order[(size_t)trial * K.nslot + q];
        if (s < 0 || s >= K.nbcap || s >= K.e_nb[env]) return it;
        if (K.alive && s >= K.first_box && s < K.first_box + K.nbox && !K.alive[(size_t)env * BD_MAXBOX + (s - K.first_box)]) return it;
        const int nv = K.sc_nv[(size_t)trial * K.nbcap + s];
        if (nv < 2 || nv > BP_MAXV) return it;
        it.kind = nv == 2 ? 1 : 0; it.nv = nv; it.rgb = K.rgb[(size_t)trial * K.nslot + s]; it.src = 0; it.idx = s;
        if (nv == 2) it.h = K.sc_prop[(size_t)trial * K.nbcap + s].x * K.scale;
        return it;
    } else if (j < K.nunder + K.nslot + nseg) {
        it.kind = 1; it.nv = 2; it.rgb = 0x0000FFu; it.h = K.path_half; it.src = 2; it.idx = j - K.nunder - K.nslot;
        return it;
    } else p = K.nunder + (j - K.nunder - K.nslot - nseg);
    const bp_render_prim &P = K.prims[p];
    if (P.kind == 0 && P.nv >= 3 && P.nv <= BP_RENDER_PRIM_VERTS) { it.kind = 0; it.nv = P.nv; }
    else if (P.kind == 1) { it.kind = 1; it.nv = 2; it.h = P.half_px + P.half_world * K.scale; }
    else return it;
    it.rgb = P.rgb; it.src = 1; it.idx = p;
    return it;
}

// vertex q of an item in frame pixels: col = (x + tx) * scale + cx, row = cy - (y + ty) * scale
__device__ __forceinline__ void render_vert(const RenderK &K, int env, int f, const RItem &it, int q, double &col, double &row)
{
    double x, y;
    if (it.src == 0) { const d2 v = K.wv[((size_t)env * K.nbcap + it.idx) * BP_MAXV + q]; x = v.x; y = v.y; }
    else if (it.src == 1) { x = K.prims[it.idx].v[q][0]; y = K.prims[it.idx].v[q][1]; }
    else { const double *pp = K.paths + ((size_t)f * K.max_path + it.idx + q) * 2; x = pp[0]; y = pp[1]; }
    col = (x + K.tx) * K.scale + K.cx;
    row = K.cy - (y + K.ty) * K.scale;
}

// capsule rule of the frame (render.py): binary64, in this order
__device__ __forceinline__ bool render_capsule(double ax, double ay, double bx, double by, double h, double px, double py)
{
    const double dx = bx - ax, dy = by - ay;
    const double dd = dx * dx + dy * dy;
    double t = 0.0;
    if (dd != 0.0) {
        t = ((px - ax) * dx + (py - ay) * dy) / dd;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double qx = ax + t * dx, qy = ay + t * dy;
    const double ex = px - qx, ey = py - qy;
    return ex * ex + ey * ey <= h * h;
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render(const RenderK K)
{
    __shared__ int s_list[RENDER_THREADS];      // surviving candidates of this pass, in draw order
    __shared__ int s_off[RENDER_THREADS];       // their first staged vertex, -1 = not staged
    __shared__ double4 s_bb[RENDER_THREADS];    // their pixel bounding boxes (c0, r0, c1, r1)
    __shared__ int s_wcnt[RENDER_THREADS / 64 + 1];
    __shared__ double s_x[RENDER_VCAP], s_y[RENDER_VCAP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fl = blockIdx.x / K.tiles, tile = blockIdx.x - fl * K.tiles;
    const int f = K.frame0 + fl;
    const int env = K.env_ids[f];
    if (env < 0 || env >= K.num_envs) return;
    const int trial = K.e_trial[env];
    if (trial < 0 || trial >= K.num_trials) return;
    int plen = 0;
    if (K.paths && K.path_len) { plen = K.path_len[f]; plen = plen < 0 ? 0 : (plen > K.max_path ? K.max_path : plen); }
    const int nseg = plen >= 2 ? plen - 1 : 0;
    const int ncand = K.nunder + K.nslot + nseg + K.nover;
    const int tyi = tile / K.tiles_x, txi = tile - tyi * K.tiles_x;
    const int c0 = txi * RENDER_TW, r0 = tyi * RENDER_TH;
    const int c1 = min(c0 + RENDER_TW, K.width) - 1, r1 = min(r0 + RENDER_TH, K.height) - 1;
    const int row = r0 + (tid >> 4), col0 = c0 + (tid & 15) * 4;
    const double py = (double)row;
    unsigned colour[4];
    unsigned pending = 0;           // bit i: pixel col0 + i is inside the frame and not yet claimed
    for (int i = 0; i < 4; i++) {
        colour[i] = K.background;
        if (row <= r1 && col0 + i <= c1) pending |= 1u << i;
    }
    const double tc0 = (double)c0 - RENDER_MARGIN, tc1 = (double)c1 + RENDER_MARGIN, tr0 = (double)r0 - RENDER_MARGIN, tr1 = (double)r1 + RENDER_MARGIN;
    int hi = ncand;
    while (hi > 0) {
        const int lo = hi > RENDER_THREADS ? hi - RENDER_THREADS : 0;
        // cull: candidate lo + tid against the tile
        const int j = lo + tid;
        bool keep = false;
        double4 bb;
        if (j < hi) {
            const RItem it = render_item(K, env, trial, plen, j);
            if (it.kind >= 0) {
                double mnc = 1e300, mnr = 1e300, mxc = -1e300, mxr = -1e300;
                for (int q = 0; q < it.nv; q++) {
                    double vc, vr;
                    render_vert(K, env, f, it, q, vc, vr);
                    mnc = fmin(mnc, vc); mxc = fmax(mxc, vc); mnr = fmin(mnr, vr); mxr = fmax(mxr, vr);
                }
                const double hh = it.kind == 1 ? it.h : 0.0;
                bb.x = mnc - hh - RENDER_MARGIN; bb.y = mnr - hh - RENDER_MARGIN; bb.z = mxc + hh + RENDER_MARGIN; bb.w = mxr + hh + RENDER_MARGIN;
                keep = bb.x <= tc1 && bb.z >= tc0 && bb.y <= tr1 && bb.w >= tr0;
            }
        }
        // order-keeping compaction
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < RENDER_THREADS / 64; w++) { if (w < wave) base += s_wcnt[w]; total += s_wcnt[w]; }
        if (keep) {
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            s_list[pos] = j; s_bb[pos] = bb;
        }
        __syncthreads();
        // stage vertices: offsets by a prefix over the survivors (one lane walks them: a pass keeps few items per tile)
        if (tid == 0) {
            int off = 0;
            for (int i = 0; i < total; i++) {
                const RItem it = render_item(K, env, trial, plen, s_list[i]);
                if (off + it.nv <= RENDER_VCAP) { s_off[i] = off; off += it.nv; } else s_off[i] = -1;
            }
        }
        __syncthreads();
        for (int i = wave; i < total; i += RENDER_THREADS / 64) {
            const int off = s_off[i];
            if (off < 0) continue;
            const RItem it = render_item(K, env, trial, plen, s_list[i]);
            for (int q = lane; q < it.nv; q += 64) render_vert(K, env, f, it, q, s_x[off + q], s_y[off + q]);
        }
        __syncthreads();
        // pixels: the first survivor from the top that covers them
        if (pending) {
            for (int i = total - 1; i >= 0 && pending; i--) {
                const double4 b = s_bb[i];
                if (py < b.y || py > b.w) continue;
                const int off = s_off[i];
                RItem it; bool have = false;
                double lx[BP_MAXV], ly[BP_MAXV];
                for (int p = 0; p < 4; p++) {
                    if (!((pending >> p) & 1u)) continue;
                    const double px = (double)(col0 + p);
                    if (px < b.x || px > b.z) continue;
                    if (!have) {
                        it = render_item(K, env, trial, plen, s_list[i]);
                        have = true;
                        if (off < 0) for (int q = 0; q < it.nv; q++) render_vert(K, env, f, it, q, lx[q], ly[q]);
                    }
                    const double *xs = off < 0 ? lx : s_x + off, *ys = off < 0 ? ly : s_y + off;
                    const bool cov = it.kind == 1 ? render_capsule(xs[0], ys[0], xs[1], ys[1], it.h, px, py) : pip_arrays(xs, ys, it.nv, px, py);
                    if (cov) { colour[p] = it.rgb; pending &= ~(1u << p); }
                }
            }
        }
        if (!__syncthreads_or(pending != 0)) break;
        hi = lo;
    }
    // store: 4 RGB pixels = 3 dwords when they are all inside the row and the address is 4-byte aligned
    if (row > r1 || col0 > c1) return;
    const size_t o = (((size_t)f * K.height + row) * K.width + col0) * 3;
    unsigned char *dst = K.out + o;
    if (col0 + 3 <= c1 && (o & 3) == 0) {
        const unsigned a = colour[0], b = colour[1], c = colour[2], d = colour[3];
        unsigned *w = (unsigned *)dst;
        w[0] = (a & 0xFFFFFFu) | (b << 24);
        w[1] = ((b >> 8) & 0xFFFFu) | (c << 16);
        w[2] = ((c >> 16) & 0xFFu) | (d << 8);
        return;
    }
    for (int p = 0; p < 4 && col0 + p <= c1; p++) {
        dst[3 * p] = (unsigned char)(colour[p] & 0xFFu);
        dst[3 * p + 1] = (unsigned char)((colour[p] >> 8) & 0xFFu);
        dst[3 * p + 2] = (unsigned char)((colour[p] >> 16) & 0xFFu);
    }
}
