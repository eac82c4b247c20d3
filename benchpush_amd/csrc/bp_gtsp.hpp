// The GTSP push planner (bp_gtsp_plan) and the controller that follows its path (bp_gtsp_track): the reference's planning-based area-clearing
// baseline (baselines/area_clearing/planning_based/policy.py: plan_path, act; GTSPPlanner/transition_graph_lookup.py; GTSPPlanner/create_instance.py)
// for every env in one launch, with an exact set DP where the reference calls the GLNS heuristic.  DESIGN.md ("GTSP") states the semantics and the
// deviations; tests/gtsp_ref.py restates them in scalar Python, and the kernels are held to == against it.
//
// k_gtsp_plan: one wavefront (= one workgroup of 64 threads) per env.
//   boxes    lane b takes box slot b: non-finite scan, the separating-axis test against the boundary, and one run of the shrink to see whether the
//            box vanishes.  A ballot gives the pushed boxes; cluster c is the c-th of them in slot order.
//   routes   lane k (and k + 64) takes node k = c * G + g: shrinks box c again (private arrays; the same arithmetic, so the same polygon), finds the
//            nearest pair with goal segment g and stores the rounded route [extended start, box point, goal point] in LDS.
//   weights  entry (u, v) of the integer matrix per lane, 64 at a time, into LDS (row stride N) and, if asked for, into global memory.
//   solve    h[S][v] for the sets S in ascending numeric order, one set per step: lane v (and v + 64) takes the minimum over the nodes u of the
//            clusters of S of W[v][u] + h[S - c(u)][u].  h lives in the caller's workspace as int32 [2^n][n * G]; a set reads only smaller sets, all
//            of them stored before the workgroup barrier (the workgroup is this one wave) that ends their step.
//   output   the tour is read forward from (all clusters, robot): the lanes test one candidate u each, the lowest set bit of the ballot is the
//            smallest u that attains h.  All lanes compute the path alike; lane 0 stores.  The tracker's first setpoint is taken on the LDS copy.
// Every loop is bounded by the caps (n <= 12, G <= 8, N <= 97, 2^n sets, BP_MAXV vertices); no atomics, no waits on other waves, plain vector loads
// and stores.  LDS: N_max^2 int32 + 3 * n_max * G + 2 * n_max + 1 double2, 42 KB at the caps.
#pragma once
#include "bp_boxdelivery.hpp"   // bd_atan2
#include "bp_rrt.hpp"           // rrt_seg_meet, rrt_orient

#define GTSP_PV (2 * BP_MAXV)    // vertices of a polygon while it is clipped: every half-plane adds one at most

extern __shared__ double2 gtsp_smem[];

struct GtspArgs {
    bp_gtsp_config c;
    double round_scale;              // 10^round_decimals
    int B, V, G, nb;                 // box slots, vertices per slot, goal segments, boundary vertices
    int n_max, N_max;                // c.max_boxes, n_max * G + 1
    long long ws_per_env;            // bytes
    double boundary[8][2];
    const double *poses, *boxes, *goals;
    const int *counts;
    const unsigned char *active;
    char *ws;
    int *status, *n_push, *tour, *cost, *lengths, *track_id, *W;
    double *paths, *track_sp;
};

__device__ __forceinline__ bool gtsp_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ double2 gtsp_ld(const double *p, int i) { return double2{p[2 * i], p[2 * i + 1]}; }

// twice the signed area, summed in vertex order
template <class F> __device__ __forceinline__ double gtsp_area2(F at, int m)
{
    double s = 0.0;
    for (int i = 0; i < m; i++) { const double2 p = at(i), q = at(i + 1 < m ? i + 1 : 0); s += p.x * q.y - q.x * p.y; }
    return s;
}
// an edge of a has all of b strictly on its outer side
template <class FA, class FB> __device__ __forceinline__ bool gtsp_sep(FA a, int na, FB b, int nb)
{
    const double o = gtsp_area2(a, na) > 0.0 ? 1.0 : -1.0;
    for (int i = 0; i < na; i++) {
        const double2 p = a(i), q = a(i + 1 < na ? i + 1 : 0);
        const double ex = q.x - p.x, ey = q.y - p.y;
        bool all = true;
        for (int k = 0; k < nb; k++) { const double2 r = b(k); all = all && (ex * (r.y - p.y) - ey * (r.x - p.x)) * o < 0.0; }
        if (all) return true;
    }
    return false;
}
// the exact inward offset by d of the convex polygon pv[0 .. m-1]: clipped by every edge's half-plane moved inwards.  Returns the vertex count (the
// polygon is in *out, which is buf0 or buf1), 0 if nothing is left
__device__ inline int gtsp_shrink(const double *pv, int m, double d, double2 *buf0, double2 *buf1, double2 **out)
{
    auto at = [&](int i) { return gtsp_ld(pv, i); };
    const double area = gtsp_area2(at, m);
    if (area == 0.0) return 0;
    const double o = area > 0.0 ? 1.0 : -1.0;
    double2 *cur = buf0, *nxt = buf1;
    int n = m;
    for (int i = 0; i < m; i++) cur[i] = at(i);
    for (int i = 0; i < m; i++) {
        const double2 a = at(i), b = at(i + 1 < m ? i + 1 : 0);
        const double ex = b.x - a.x, ey = b.y - a.y;
        const double L = __builtin_sqrt(ex * ex + ey * ey);
        if (L == 0.0) continue;
        const double nx = (o * -ey) / L, ny = (o * ex) / L;
        int cnt = 0;
        for (int k = 0; k < n; k++) {
            const double2 P = cur[k], Q = cur[k + 1 < n ? k + 1 : 0];
            const double fp = ((P.x - a.x) * nx + (P.y - a.y) * ny) - d, fq = ((Q.x - a.x) * nx + (Q.y - a.y) * ny) - d;
            if (fp >= 0.0) { if (cnt < GTSP_PV) nxt[cnt] = P; cnt++; }
            if ((fp >= 0.0) != (fq >= 0.0)) {
                const double t = fp / (fp - fq);
                if (cnt < GTSP_PV) nxt[cnt] = double2{P.x + t * (Q.x - P.x), P.y + t * (Q.y - P.y)};
                cnt++;
            }
        }
        if (cnt < 3 || cnt > GTSP_PV) return 0;
        double2 *t = cur; cur = nxt; nxt = t;
        n = cnt;
    }
    auto ac = [&](int i) { return cur[i]; };
    if (!(gtsp_area2(ac, n) * o > 0.0)) return 0;
    *out = cur;
    return n;
}
// the point of the segment (a, b) nearest p, and the squared distance
__device__ __forceinline__ double2 gtsp_proj(double2 p, double2 a, double2 b, double &d2)
{
    const double abx = b.x - a.x, aby = b.y - a.y, apx = p.x - a.x, apy = p.y - a.y;
    const double l2 = abx * abx + aby * aby;
    double2 q = a;
    if (l2 != 0.0) {
        double t = (apx * abx + apy * aby) / l2;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        q = double2{a.x + t * abx, a.y + t * aby};
    }
    const double ex = p.x - q.x, ey = p.y - q.y;
    d2 = ex * ex + ey * ey;
    return q;
}
__device__ __forceinline__ double gtsp_rnd(double v, double scale) { return __builtin_rint(v * scale) / scale; }
// the route [extended start, box point, goal point] of pushing the box pv (shrunk: poly) to the goal segment (g0, g1); true if it is degenerate
__device__ inline bool gtsp_route(const double *pv, int m, const double2 *poly, int n, double2 g0, double2 g1, double extend, double scale, double2 *r)
{
    bool touch = false, pos = false, neg = false;
    for (int j = 0; j < n; j++) {
        const double2 a = poly[j], b = poly[j + 1 < n ? j + 1 : 0];
        touch = touch || rrt_seg_meet(a, b, g0, g1);
        const double o = rrt_orient(a, b, g0);
        pos = pos || o > 0.0; neg = neg || o < 0.0;
    }
    double d2;
    if (touch || !(pos && neg)) {
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < m; i++) { sx += pv[2 * i]; sy += pv[2 * i + 1]; }
        double2 q = gtsp_proj(double2{sx / (double)m, sy / (double)m}, g0, g1, d2);
        q = double2{gtsp_rnd(q.x, scale), gtsp_rnd(q.y, scale)};
        r[0] = q; r[1] = q; r[2] = q;
        return true;
    }
    double best = 0.0;
    double2 bp = poly[0], gp = g0;
    for (int i = 0; i < n; i++) {
        const double2 q = gtsp_proj(poly[i], g0, g1, d2);
        if (i == 0 || d2 < best) { best = d2; bp = poly[i]; gp = q; }
    }
    for (int e = 0; e < 2; e++) {
        const double2 ge = e == 0 ? g0 : g1;
        for (int j = 0; j < n; j++) {
            const double2 q = gtsp_proj(ge, poly[j], poly[j + 1 < n ? j + 1 : 0], d2);
            if (d2 < best) { best = d2; bp = q; gp = ge; }
        }
    }
    const double dx = bp.x - gp.x, dy = bp.y - gp.y;
    const double L = __builtin_sqrt(dx * dx + dy * dy);
    double2 ext = bp;
    if (L != 0.0) ext = double2{bp.x + (dx / L) * extend, bp.y + (dy / L) * extend};
    r[0] = double2{gtsp_rnd(ext.x, scale), gtsp_rnd(ext.y, scale)};
    r[1] = double2{gtsp_rnd(bp.x, scale), gtsp_rnd(bp.y, scale)};
    r[2] = double2{gtsp_rnd(gp.x, scale), gtsp_rnd(gp.y, scale)};
    return false;
}
__device__ __forceinline__ double gtsp_angle(double2 a, double2 b)
{
    if (__builtin_sqrt(a.x * a.x + a.y * a.y) == 0.0 || __builtin_sqrt(b.x * b.x + b.y * b.y) == 0.0) return 0.0;
    return __builtin_fabs(bd_atan2(a.x * b.y - a.y * b.x, a.x * b.x + a.y * b.y));
}

__global__ __launch_bounds__(64) void k_gtsp_plan(const GtspArgs A)
{
    const int lane = (int)threadIdx.x;
    const size_t env = blockIdx.x;
    if (A.active && !A.active[env]) { if (lane == 0) A.status[env] = BP_GTSP_SKIPPED; return; }
    const bp_gtsp_config &c = A.c;
    const int B = A.B, V = A.V, G = A.G, n_max = A.n_max, N_max = A.N_max, P = 2 * n_max + 1;
    int *Wl = (int *)gtsp_smem;                                                   // [N][N], N <= N_max
    double2 *rt = gtsp_smem + ((size_t)N_max * N_max + 3) / 4;                    // [n_max * G][3]
    double2 *pl = rt + (size_t)n_max * G * 3;                                     // [P] the path's (x, y)
    int *h = (int *)(A.ws + env * (size_t)A.ws_per_env);
    double *path = A.paths + env * (size_t)P * 3;
    const double x = A.poses[3 * env], y = A.poses[3 * env + 1], th = A.poses[3 * env + 2];
    double2 buf0[GTSP_PV], buf1[GTSP_PV], *poly = buf0;

    // ---- boxes: non-finite scan, which are pushed, which vanish ----
    bool bad = !(gtsp_finite(x) && gtsp_finite(y) && gtsp_finite(th));
    for (int i = lane; i < 4 * G; i += 64) bad = bad || !gtsp_finite(A.goals[i]);
    bool push = false, gone = false;
    if (lane < B) {
        const int cnt = A.counts[env * (size_t)B + lane];
        const double *pv = A.boxes + (env * (size_t)B + lane) * (size_t)V * 2;
        if (cnt != 0 && (cnt < 3 || cnt > V)) bad = true;
        else if (cnt != 0) {
            for (int i = 0; i < 2 * cnt; i++) bad = bad || !gtsp_finite(pv[i]);
            if (!bad) {
                auto bx = [&](int i) { return gtsp_ld(pv, i); };
                auto bd = [&](int i) { return double2{A.boundary[i][0], A.boundary[i][1]}; };
                if (!(gtsp_sep(bd, A.nb, bx, cnt) || gtsp_sep(bx, cnt, bd, A.nb))) {
                    push = gtsp_shrink(pv, cnt, c.shrink, buf0, buf1, &poly) > 0;
                    gone = !push;
                }
            }
        }
    }
    if (ballot(bad) != 0ull) {
        if (lane == 0) { A.status[env] = BP_GTSP_INVALID; A.n_push[env] = 0; A.cost[env] = 0; A.lengths[env] = 0; }
        return;
    }
    const unsigned long long pmask = ballot(push);
    const int n = (int)__popcll(pmask);
    int flags = ballot(gone) != 0ull ? BP_GTSP_FLAG_VANISHED : 0;
    if (n > n_max) {
        if (lane == 0) { A.status[env] = BP_GTSP_CAP | flags; A.n_push[env] = n; A.cost[env] = 0; A.lengths[env] = 0; }
        return;
    }
    const int R = n * G, N = R + 1;      // the robot is node R

    // ---- routes: one node per lane ----
    bool deg = false;
    for (int k = lane; k < R; k += 64) {
        const int cl = k / G, g = k - cl * G;
        unsigned long long mm = pmask;
        for (int i = 0; i < cl; i++) mm &= mm - 1;
        const int b = (int)__builtin_ctzll(mm);
        const int cnt = A.counts[env * (size_t)B + b];
        const double *pv = A.boxes + (env * (size_t)B + b) * (size_t)V * 2;
        const int np = gtsp_shrink(pv, cnt, c.shrink, buf0, buf1, &poly);
        double2 r[3];
        deg = gtsp_route(pv, cnt, poly, np, gtsp_ld(A.goals, 2 * g), gtsp_ld(A.goals, 2 * g + 1), c.extend, A.round_scale, r) || deg;
        rt[3 * k] = r[0]; rt[3 * k + 1] = r[1]; rt[3 * k + 2] = r[2];
    }
    if (ballot(deg) != 0ull) flags |= BP_GTSP_FLAG_DEGENERATE;
    __syncthreads();

    // ---- weights ----
    double sn, cs;
    bp_sincos(th, sn, cs);
    const double2 rob = {x, y}, rdir = {(x + 0.1 * cs) - x, (y + 0.1 * sn) - y};
    for (int idx = lane; idx < N * N; idx += 64) {
        const int u = idx / N, v = idx - u * N;
        int w;
        if (u == v) w = 99999999;
        else if (u != R && v != R && u / G == v / G) w = 0;
        else {
            const double2 du = u == R ? rdir : double2{rt[3 * u + 2].x - rt[3 * u + 1].x, rt[3 * u + 2].y - rt[3 * u + 1].y};
            const double2 dv = v == R ? rdir : double2{rt[3 * v + 2].x - rt[3 * v + 1].x, rt[3 * v + 2].y - rt[3 * v + 1].y};
            const double2 frm = u == R ? rob : rt[3 * u + 2], to = v == R ? rob : rt[3 * v];
            const double2 p = {to.x - frm.x, to.y - frm.y};
            const double ln = __builtin_sqrt(p.x * p.x + p.y * p.y);
            const double an = gtsp_angle(du, p) + gtsp_angle(p, dv);
            const double cost = c.lin_vel * ln + c.ang_vel * an;
            const double wf = __builtin_rint(100.0 * cost);
            w = wf < 99999999.0 ? (int)wf : 99999999;
        }
        Wl[idx] = w;
        if (A.W) A.W[(env * (size_t)N_max + u) * (size_t)N_max + v] = w;
    }
    __syncthreads();

    // ---- solve: h[S][v], S ascending ----
    int cost = 0;
    if (n > 0) {
        const int v0 = lane, v1 = lane + 64;
        const int c0 = v0 < R ? v0 / G : -1, c1 = v1 < R ? v1 / G : -1;
        if (c0 >= 0) h[v0] = Wl[v0 * N + R];
        if (c1 >= 0) h[v1] = Wl[v1 * N + R];
        __syncthreads();
        const int full = (1 << n) - 1;
        for (int S = 1; S <= full; S++) {
            const bool do0 = c0 >= 0 && !((S >> c0) & 1), do1 = c1 >= 0 && !((S >> c1) & 1);
            int b0 = 0x7FFFFFFF, b1 = 0x7FFFFFFF;
            for (int m = S; m != 0; m &= m - 1) {
                const int cu = __builtin_ctz(m);
                const int *hs = h + (size_t)(S ^ (1 << cu)) * R + cu * G;
                for (int g = 0; g < G; g++) {
                    const int hv = hs[g], u = cu * G + g;
                    if (do0) { const int t = Wl[v0 * N + u] + hv; b0 = t < b0 ? t : b0; }
                    if (do1) { const int t = Wl[v1 * N + u] + hv; b1 = t < b1 ? t : b1; }
                }
            }
            if (do0) h[(size_t)S * R + v0] = b0;
            if (do1) h[(size_t)S * R + v1] = b1;
            __syncthreads();       // the set's values are in memory before a larger set reads them
        }
        // ---- the tour, forward from (all clusters, robot) ----
        int S = full, cur = R, target = 0;
        for (int step = 0; step <= n && S != 0; step++) {
            int t0 = 0x7FFFFFFF, t1 = 0x7FFFFFFF;
            if (c0 >= 0 && ((S >> c0) & 1)) t0 = Wl[cur * N + v0] + h[(size_t)(S ^ (1 << c0)) * R + v0];
            if (c1 >= 0 && ((S >> c1) & 1)) t1 = Wl[cur * N + v1] + h[(size_t)(S ^ (1 << c1)) * R + v1];
            if (step == 0) {
                int t = t0 < t1 ? t0 : t1;
                for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(t, m); t = o < t ? o : t; }
                target = cost = t;
            }
            const unsigned long long m0 = ballot(t0 == target), m1 = ballot(t1 == target);
            if ((m0 | m1) == 0ull) break;          // cannot happen: some successor attains h
            const int u = m0 != 0ull ? (int)__builtin_ctzll(m0) : 64 + (int)__builtin_ctzll(m1);
            S ^= 1 << (u / G);
            target = h[(size_t)S * R + u];
            if (lane == 0) A.tour[env * (size_t)n_max + step] = u;
            const double2 a = rt[3 * u], e = rt[3 * u + 2];
            const double hd = bd_atan2(e.y - a.y, e.x - a.x);
            if (lane == 0) {
                double *q = path + 3 * (2 * step + 1);
                q[0] = a.x; q[1] = a.y; q[2] = hd; q[3] = e.x; q[4] = e.y; q[5] = hd;
                pl[2 * step + 1] = a; pl[2 * step + 2] = e;
            }
            cur = u;
        }
    }
    if (lane == 0) { path[0] = x; path[1] = y; path[2] = th; pl[0] = rob; }
    __syncthreads();

    // ---- the tracker's first state: TargetCourse.init_setpoint on the path ----
    const int len = 2 * n + 1;
    double bd = BP_INF;
    int bi = 0x7FFFFFFF;
    if (lane < len) { const double dx = x - pl[lane].x, dy = y - pl[lane].y; bd = dx * dx + dy * dy; bi = lane; }
    for (int m = 32; m >= 1; m >>= 1) {
        const double od = __shfl_xor(bd, m);
        const int oi = __shfl_xor(bi, m);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    bool stop = false;
    if (lane >= bi && lane < len) { const double dx = x - pl[lane].x, dy = y - pl[lane].y; stop = !(c.Lfc > __builtin_sqrt(dx * dx + dy * dy)); }
    const unsigned long long sm = ballot(stop);
    const int ind = sm != 0ull ? (int)__builtin_ctzll(sm) : len - 1;
    if (lane == 0) {
        A.status[env] = (n > 0 ? BP_GTSP_OK : BP_GTSP_NOTHING_TO_PUSH) | flags;
        A.n_push[env] = n; A.cost[env] = cost; A.lengths[env] = len;
        A.track_id[env] = 1; A.track_sp[2 * env] = pl[ind].x; A.track_sp[2 * env + 1] = pl[ind].y;
    }
}

// ---- the controller ----
struct GtspTrackArgs {
    bp_gtsp_config c;
    int P;                           // rows of a path: 2 * max_boxes + 1
    const double *paths, *poses;
    const int *lengths;
    const unsigned char *active;
    int *track_id, *diag;
    double *track_sp, *actions;
};

__global__ __launch_bounds__(64) void k_gtsp_track(const GtspTrackArgs A)
{
    const int lane = (int)threadIdx.x;
    const size_t env = blockIdx.x;
    const bp_gtsp_config &c = A.c;
    const double *path = A.paths + env * (size_t)A.P * 3;
    int len = min(A.lengths[env], A.P);
    if (A.active && !A.active[env]) len = 0;
    const double x = A.poses[3 * env], y = A.poses[3 * env + 1], yaw = A.poses[3 * env + 2];
    int id = A.track_id[env];
    double sx = A.track_sp[2 * env], sy = A.track_sp[2 * env + 1];
    bool bad = !(gtsp_finite(x) && gtsp_finite(y) && gtsp_finite(yaw)) || id < 0;
    for (int i = lane; i < 3 * len; i += 64) if (!gtsp_finite(path[i])) bad = true;
    if (len < 2 || ballot(bad) != 0ull) {
        if (lane == 0) { A.actions[2 * env] = __builtin_nan(""); A.actions[2 * env + 1] = __builtin_nan(""); A.diag[env] = -1; }
        return;
    }
    bool done = id >= len;
    if (!done) {
        const double dx = x - path[3 * id], dy = y - path[3 * id + 1];
        if (__builtin_sqrt(dx * dx + dy * dy) < c.switch_dist) {
            id++;
            done = id >= len;
            if (!done) { sx = path[3 * id]; sy = path[3 * id + 1]; }
        }
    }
    double speed = 0.0, omega = 0.0;
    if (!done) {
        const double theta_d = bd_atan2(sy - y, sx - x);
        double sn, cs;
        bp_sincos(theta_d - yaw, sn, cs);
        omega = bd_atan2(sn, cs) / c.dt / c.w_scale;
        bp_sincos(yaw, sn, cs);
        const double vx = cs * c.target_speed, vy = sn * c.target_speed;
        speed = __builtin_sqrt(vx * vx + vy * vy) / c.v_scale;
    }
    if (lane == 0) {
        A.actions[2 * env] = speed; A.actions[2 * env + 1] = omega; A.diag[env] = id;
        A.track_id[env] = id; A.track_sp[2 * env] = sx; A.track_sp[2 * env + 1] = sy;
    }
}
