// Batched RRT (bp_rrt_plan) and the waypoint controller that follows its paths (bp_track_waypoints): the reference's planning-based maze-NAMO baseline
// (baselines/maze_NAMO/planning_based/RRT/rrt.py: RRTPlanner.plan / _run_rrt / _steer / _backtrack / _densify; policy.py: prune_by_distance and act with
// common/controller/dp.py: DP.ideal_control) for every env in one launch.  DESIGN.md ("RRT") states the semantics and the deviations;
// tests/rrt_ref.py restates them in scalar Python, and the kernels are held to == against it.
//
// k_rrt_plan: one wavefront (= one workgroup of 64 threads) per env.
//   setup   the walls and the edges of the counted box polygons go to LDS as segments (a, b), the polygons as (first edge, edges); the lanes scan all
//           inputs for a non-finite value, reduce the sampling bounds and test start and goal against the inflated walls.
//   search  per iteration all lanes draw the same sample from the counter RNG; each lane keeps the smallest (d2, index) of the nodes lane, lane + 64, ...
//           (16-byte loads), a butterfly leaves the smallest key -- lowest index among equals -- in all lanes; the steered segment is tested against 64
//           LDS segments per round (exact capsule test for walls, closed orientation tests for box edges), then against the polygons' insides; every
//           verdict is a ballot, so all branches are wave-uniform.  Lane 0 appends.
//   output  the path is walked through the parents, which are reversed along it for the walk and restored after it; _densify and prune_by_distance run
//           over that stream of points (two walks: the first finds the last dense point, which the pruning rule needs from the start).
// The search and the walks along the parents are bounded by max_nodes; _densify's points by the host check (max_nodes + 2) * points per edge <=
// RRT_DENSE_POINTS_MAX.  No atomics, no waits on other waves, plain vector loads and stores.  The tree lives in the caller's workspace: per env
// (max_nodes + 2) nodes as double2, then as many int32 parents.  The first lds_nodes nodes (a multiple of 64, 0: none) are mirrored in LDS and the
// nearest search reads them from there: the same values in the same order, so the plan does not depend on it (profiles/rrt/README.md has the timing).
// Global memory that lane 0 stores and all lanes load later is ordered by a workgroup barrier (the workgroup is this one wave) wherever the load can
// follow the store to the same address; a load that precedes the store to its address needs none, the wave's memory operations issue in order.
#pragma once
#include "bp_boxdelivery.hpp"   // bd_atan2

#define RRT_DENSE_POINTS_MAX 4194304.0   // host check: (max_nodes + 2) * max(1, max(step, goal_radius) / max(1e-3, densify_ds)) stays within this: all of _densify's points

#define RRT_LDS_NODES_DEFAULT 512         // nodes of the tree that the nearest search keeps in LDS unless BP_RRT_LDS_NODES says otherwise

extern __shared__ double2 rrt_smem[];

struct RrtArgs {
    bp_rrt_config c;
    int W, B, V, lds_nodes;
    long long ws_per_env;            // bytes
    const double *starts, *goals, *walls, *boxes;
    const int *counts;
    const long long *streams;
    const unsigned char *active;
    char *ws;
    int *status, *n_nodes, *iterations, *lengths;
    double *paths;
};

__host__ __device__ inline double bp_rrt_u01(unsigned long long seed, long long stream, int p, int k, int j)
{
    const unsigned long long key = bp_splitmix64(seed ^ bp_splitmix64((unsigned long long)stream));
    const unsigned long long z = bp_splitmix64(key ^ (((unsigned long long)(p & 3) << 62) | ((unsigned long long)(unsigned)k << 2) | (unsigned long long)(j & 3)));
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ bool rrt_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ double rrt_orient(double2 a, double2 b, double2 c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x); }
__device__ __forceinline__ bool rrt_on(double2 a, double2 b, double2 c)
{
    return (a.x < b.x ? a.x : b.x) <= c.x && c.x <= (a.x > b.x ? a.x : b.x) && (a.y < b.y ? a.y : b.y) <= c.y && c.y <= (a.y > b.y ? a.y : b.y);
}
// do the closed segments (a, b) and (c, d) share a point?
__device__ __forceinline__ bool rrt_seg_meet(double2 a, double2 b, double2 c, double2 d)
{
    const double o1 = rrt_orient(a, b, c), o2 = rrt_orient(a, b, d), o3 = rrt_orient(c, d, a), o4 = rrt_orient(c, d, b);
    if (((o1 > 0 && o2 < 0) || (o1 < 0 && o2 > 0)) && ((o3 > 0 && o4 < 0) || (o3 < 0 && o4 > 0))) return true;
    if (o1 == 0 && rrt_on(a, b, c)) return true;
    if (o2 == 0 && rrt_on(a, b, d)) return true;
    if (o3 == 0 && rrt_on(c, d, a)) return true;
    if (o4 == 0 && rrt_on(c, d, b)) return true;
    return false;
}
__device__ __forceinline__ double rrt_point_seg_d2(double2 p, double2 a, double2 b)
{
    const double abx = b.x - a.x, aby = b.y - a.y, apx = p.x - a.x, apy = p.y - a.y;
    const double l2 = abx * abx + aby * aby;
    if (l2 == 0.0) return apx * apx + apy * apy;
    double t = (apx * abx + apy * aby) / l2;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double ex = p.x - (a.x + t * abx), ey = p.y - (a.y + t * aby);
    return ex * ex + ey * ey;
}
__device__ __forceinline__ double rrt_seg_seg_d2(double2 a, double2 b, double2 c, double2 d)
{
    if (rrt_seg_meet(a, b, c, d)) return 0.0;
    double m = rrt_point_seg_d2(a, c, d);
    double v = rrt_point_seg_d2(b, c, d); m = v < m ? v : m;
    v = rrt_point_seg_d2(c, a, b); m = v < m ? v : m;
    v = rrt_point_seg_d2(d, a, b); m = v < m ? v : m;
    return m;
}
// the lane's share of the nearest search over nodes[i], i = first, first + 64, ... below end: ascending, so the lowest index wins among equals
__device__ __forceinline__ void rrt_scan(const double2 *nodes, int first, int end, double2 q, double &bd, int &bi)
{
    int i = first;
    for (; i + 192 < end; i += 256) {
        const double2 n0 = nodes[i], n1 = nodes[i + 64], n2 = nodes[i + 128], n3 = nodes[i + 192];
        const double x0 = n0.x - q.x, y0 = n0.y - q.y, x1 = n1.x - q.x, y1 = n1.y - q.y, x2 = n2.x - q.x, y2 = n2.y - q.y, x3 = n3.x - q.x, y3 = n3.y - q.y;
        const double d0 = x0 * x0 + y0 * y0, d1 = x1 * x1 + y1 * y1, d2 = x2 * x2 + y2 * y2, d3 = x3 * x3 + y3 * y3;
        if (d0 < bd) { bd = d0; bi = i; }
        if (d1 < bd) { bd = d1; bi = i + 64; }
        if (d2 < bd) { bd = d2; bi = i + 128; }
        if (d3 < bd) { bd = d3; bi = i + 192; }
    }
    for (; i < end; i += 64) {
        const double2 nd = nodes[i];
        const double dx = nd.x - q.x, dy = nd.y - q.y, d2 = dx * dx + dy * dy;
        if (d2 < bd) { bd = d2; bi = i; }
    }
}
__device__ __forceinline__ double rrt_wave_min(double v) { for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m); v = o < v ? o : v; } return v; }
__device__ __forceinline__ double rrt_wave_max(double v) { for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m); v = o > v ? o : v; } return v; }

// The dense stream of the found path (_densify over _backtrack), walked through `next` (the reversed parents) from node 0.  WRITE false: returns the
// number of dense points and their last one.  WRITE true: prune_by_distance over the stream (n_dense, fin from the first walk); returns the number of
// waypoints, the last one included, and stores the first P of them.
template <bool WRITE>
__device__ __forceinline__ int rrt_walk(const double2 *nodes, const int *next, int n_tree, double ds, double min_dist, int n_dense, double2 &fin,
                                        double *path, int P, int lane)
{
    double2 a = nodes[0], prev = a;
    int count = 1, kept = 1, idx = next[0];
    if (WRITE && lane == 0) { path[0] = a.x; path[1] = a.y; }
    for (int guard = 0; guard < n_tree && idx >= 0; guard++) {
        const double2 b = nodes[idx];
        const double ex = b.x - a.x, ey = b.y - a.y;
        const double q = __builtin_sqrt(ex * ex + ey * ey) / ds;
        int n = q < RRT_DENSE_POINTS_MAX ? (int)q : (int)RRT_DENSE_POINTS_MAX;
        n = n < 1 ? 1 : n;
        double2 pt = a;
        for (int k = 1; k <= n; k++) {
            const double t = (double)k / (double)n;
            pt.x = a.x + t * ex; pt.y = a.y + t * ey;
            if (WRITE && count < n_dense - 1) {       // path[1 .. N-2] of prune_by_distance
                const double px = pt.x - prev.x, py = pt.y - prev.y, fx = pt.x - fin.x, fy = pt.y - fin.y;
                if (__builtin_sqrt(px * px + py * py) >= min_dist && __builtin_sqrt(fx * fx + fy * fy) >= min_dist) {
                    if (kept < P && lane == 0) { path[2 * kept] = pt.x; path[2 * kept + 1] = pt.y; }
                    kept++;
                    prev = pt;
                }
            }
            count++;
        }
        a = pt;
        idx = next[idx];
    }
    if (!WRITE) { fin = a; return count; }
    if (kept < P && lane == 0) { path[2 * kept] = fin.x; path[2 * kept + 1] = fin.y; }
    return kept + 1;
}

__global__ __launch_bounds__(64) void k_rrt_plan(const RrtArgs A)
{
    const int lane = (int)threadIdx.x;
    const size_t env = blockIdx.x;
    if (A.active && !A.active[env]) { if (lane == 0) A.status[env] = BP_RRT_SKIPPED; return; }
    const bp_rrt_config &c = A.c;
    const int W = A.W, B = A.B, V = A.V, P = c.max_waypoints;
    double2 *seg = rrt_smem;                                  // [W + B * V][2]: a, b
    int *pfirst = (int *)(seg + 2 * (size_t)(W + B * V));     // [B] first edge of the polygon (an index into seg), [B] its edges
    int *pcnt = pfirst + B;
    const int K = A.lds_nodes;
    double2 *lnodes = (double2 *)(pcnt + B + 2 * (B & 1));    // [K] the first nodes of the tree; 2 * (B + (B & 1)) ints before it keep it 16-byte aligned
    double2 *nodes = (double2 *)(A.ws + env * (size_t)A.ws_per_env);
    int *parent = (int *)(nodes + (size_t)c.max_nodes + 2);
    double *path = A.paths + env * (size_t)P * 2;
    const double2 start = {A.starts[2 * env], A.starts[2 * env + 1]}, goal = {A.goals[2 * env], A.goals[2 * env + 1]};

    // ---- setup: segments to LDS, non-finite scan, bounds ----
    bool bad = !(rrt_finite(start.x) && rrt_finite(start.y) && rrt_finite(goal.x) && rrt_finite(goal.y));
    double xmin = BP_INF, xmax = -BP_INF, ymin = BP_INF, ymax = -BP_INF;
    for (int w = lane; w < W; w += 64) {
        const double2 a = {A.walls[4 * w], A.walls[4 * w + 1]}, b = {A.walls[4 * w + 2], A.walls[4 * w + 3]};
        seg[2 * w] = a; seg[2 * w + 1] = b;
        bad = bad || !(rrt_finite(a.x) && rrt_finite(a.y) && rrt_finite(b.x) && rrt_finite(b.y));
        xmin = a.x < xmin ? a.x : xmin; xmin = b.x < xmin ? b.x : xmin; xmax = a.x > xmax ? a.x : xmax; xmax = b.x > xmax ? b.x : xmax;
        ymin = a.y < ymin ? a.y : ymin; ymin = b.y < ymin ? b.y : ymin; ymax = a.y > ymax ? a.y : ymax; ymax = b.y > ymax ? b.y : ymax;
    }
    int nseg = W, npoly = 0;
    for (int b = 0; b < B; b++) {
        const int cnt = A.counts[env * (size_t)B + b];
        if (cnt == 0) continue;
        if (cnt < 3 || cnt > V) { bad = true; continue; }
        const double *pv = A.boxes + (env * (size_t)B + b) * (size_t)V * 2;
        for (int v = lane; v < cnt; v += 64) {
            const int v2 = v + 1 < cnt ? v + 1 : 0;
            const double2 p = {pv[2 * v], pv[2 * v + 1]}, q = {pv[2 * v2], pv[2 * v2 + 1]};
            seg[2 * (nseg + v)] = p; seg[2 * (nseg + v) + 1] = q;
            bad = bad || !(rrt_finite(p.x) && rrt_finite(p.y));
            xmin = p.x < xmin ? p.x : xmin; xmax = p.x > xmax ? p.x : xmax; ymin = p.y < ymin ? p.y : ymin; ymax = p.y > ymax ? p.y : ymax;
        }
        if (lane == 0) { pfirst[npoly] = nseg; pcnt[npoly] = cnt; }
        nseg += cnt; npoly++;
    }
    __syncthreads();
    if (ballot(bad) != 0ull) {
        if (lane == 0) {
            A.status[env] = BP_RRT_BAD_INPUT; A.lengths[env] = 0;
            A.n_nodes[2 * env] = A.n_nodes[2 * env + 1] = A.iterations[2 * env] = A.iterations[2 * env + 1] = 0;
        }
        return;
    }
    if (nseg > 0) { xmin = rrt_wave_min(xmin); xmax = rrt_wave_max(xmax); ymin = rrt_wave_min(ymin); ymax = rrt_wave_max(ymax); }
    else { xmin = -3.0; xmax = 3.0; ymin = -3.0; ymax = 3.0; }     // the reference's bounds of an empty scene
    const double r2 = c.inflate_radius * c.inflate_radius;
    bool blocked = false;
    for (int w = lane; w < W; w += 64)
        blocked = blocked || rrt_point_seg_d2(start, seg[2 * w], seg[2 * w + 1]) <= r2 || rrt_point_seg_d2(goal, seg[2 * w], seg[2 * w + 1]) <= r2;
    int status = ballot(blocked) != 0ull ? BP_RRT_BLOCKED : BP_RRT_FALLBACK;
    int nn[2] = {0, 0}, its[2] = {0, 0};

    // ---- search ----
    const double gr2 = c.goal_radius * c.goal_radius, xr = xmax - xmin, yr = ymax - ymin;
    const long long stream = A.streams[env];
    int n = 0;
    for (int p = 0; p < c.passes && status == BP_RRT_FALLBACK; p++) {
        if (lane == 0) { nodes[0] = start; parent[0] = -1; if (K > 0) lnodes[0] = start; }
        __syncthreads();
        n = 1;
        const int ntest = p == 0 ? nseg : W;     // boxes block in pass 0 only
        bool found = false;
        int k = 0;
        for (; k < c.max_nodes && !found; k++) {
            double2 q = goal;
            if (!(bp_rrt_u01(c.seed, stream, p, k, 0) < c.goal_bias)) {
                q.x = xmin + xr * bp_rrt_u01(c.seed, stream, p, k, 1);
                q.y = ymin + yr * bp_rrt_u01(c.seed, stream, p, k, 2);
            }
            // nearest node: the lowest index of the smallest d2
            double bd = BP_INF;
            int bi = 0x7FFFFFFF;
            const int nl = n < K ? n : K;                      // K is a multiple of 64: lane l goes on at K + l in global memory
            rrt_scan(lnodes, lane, nl, q, bd, bi);
            rrt_scan(nodes, K + lane, n, q, bd, bi);
            for (int m = 32; m >= 1; m >>= 1) {
                const double od = __shfl_xor(bd, m);
                const int oi = __shfl_xor(bi, m);
                if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
            }
            if (bi == 0x7FFFFFFF) bi = 0;      // no d2 below +inf: the first node, as `best is None or d < best` leaves it
            // steer
            const double2 a = nodes[bi];
            const double dx = q.x - a.x, dy = q.y - a.y, L = __builtin_sqrt(bd);
            double2 nw = q;
            if (!(L <= c.step || L == 0.0)) { const double s = c.step / L; nw.x = a.x + s * dx; nw.y = a.y + s * dy; }
            // collision
            bool hit = false;
            for (int s0 = 0; s0 < ntest; s0 += 64) {
                const int s = s0 + lane;
                bool h = false;
                if (s < W) h = rrt_seg_seg_d2(a, nw, seg[2 * s], seg[2 * s + 1]) <= r2;
                else if (s < ntest) h = rrt_seg_meet(a, nw, seg[2 * s], seg[2 * s + 1]);
                if (ballot(h) != 0ull) { hit = true; break; }
            }
            if (!hit && p == 0) {
                for (int b0 = 0; b0 < npoly; b0 += 64) {
                    const int b = b0 + lane;
                    bool h = false;
                    if (b < npoly) {
                        bool apos = false, aneg = false, npos = false, nneg = false;
                        const int f = pfirst[b], cnt = pcnt[b];
                        for (int v = 0; v < cnt; v++) {
                            const double2 ea = seg[2 * (f + v)], eb = seg[2 * (f + v) + 1];
                            const double oa = rrt_orient(ea, eb, a), on = rrt_orient(ea, eb, nw);
                            apos = apos || oa > 0; aneg = aneg || oa < 0; npos = npos || on > 0; nneg = nneg || on < 0;
                        }
                        h = !(apos && aneg) || !(npos && nneg);
                    }
                    if (ballot(h) != 0ull) { hit = true; break; }
                }
            }
            if (hit) continue;
            if (lane == 0) { nodes[n] = nw; parent[n] = bi; if (n < K) lnodes[n] = nw; }
            n++;
            const double gx = nw.x - goal.x, gy = nw.y - goal.y;
            if (gx * gx + gy * gy <= gr2) {
                if (lane == 0) { nodes[n] = goal; parent[n] = n - 1; }      // never scanned: the pass ends here
                n++;
                found = true;
            }
            __syncthreads();       // the appended node is in memory before the next scan reads it
        }
        nn[p] = n; its[p] = k;
        if (found) status = p == 0 ? BP_RRT_FOUND : BP_RRT_FOUND_IGNORING_BOXES;
    }

    // ---- output ----
    int length = 2;
    if (status == BP_RRT_FOUND || status == BP_RRT_FOUND_IGNORING_BOXES) {
        // reverse the parents along the path: parent[] becomes `next` from node 0 to the goal.  Every node is visited once: its parent is loaded (by
        // all lanes) before lane 0 stores to it, in issue order, and nothing loads it again before the barrier below
        int idx = n - 1, prv = -1;
        for (int guard = 0; guard < n && idx >= 0; guard++) {
            const int up = parent[idx];
            if (lane == 0) parent[idx] = prv;
            prv = idx; idx = up;
        }
        __syncthreads();
        const double ds = c.densify_ds > 1e-3 ? c.densify_ds : 1e-3;
        double2 fin = start;
        const int n_dense = rrt_walk<false>(nodes, parent, n, ds, c.prune_min_dist, 0, fin, path, P, lane);
        length = rrt_walk<true>(nodes, parent, n, ds, c.prune_min_dist, n_dense, fin, path, P, lane);
        if (length > P) { status = BP_RRT_CAP; length = 0; }
        // and back: the workspace keeps the tree of the pass that found the path
        idx = 0; prv = -1;
        for (int guard = 0; guard < n && idx >= 0; guard++) {
            const int down = parent[idx];     // as above: load, then store, each address once
            if (lane == 0) parent[idx] = prv;
            prv = idx; idx = down;
        }
    } else if (lane == 0) {
        path[0] = start.x; path[1] = start.y; path[2] = goal.x; path[3] = goal.y;     // [start, goal], as the reference returns
    }
    if (lane == 0) {
        A.status[env] = status; A.lengths[env] = length;
        A.n_nodes[2 * env] = nn[0]; A.n_nodes[2 * env + 1] = nn[1]; A.iterations[2 * env] = its[0]; A.iterations[2 * env + 1] = its[1];
    }
}

// ---- the waypoint controller ----
struct TrackWpArgs {
    bp_track_wp_config c;
    const double *paths, *poses;
    const int *lengths;
    const unsigned char *active;
    double *actions;
    int *diag;
};

__global__ __launch_bounds__(64) void k_track_waypoints(const TrackWpArgs A)
{
    const int lane = (int)threadIdx.x;
    const size_t env = blockIdx.x;
    const bp_track_wp_config &c = A.c;
    const double *path = A.paths + env * (size_t)c.P * 2;
    int len = A.lengths ? min(A.lengths[env], c.P) : c.P;
    if (A.active && !A.active[env]) len = 0;
    const double x = A.poses[3 * env], y = A.poses[3 * env + 1], yaw = A.poses[3 * env + 2];
    bool bad = !(rrt_finite(x) && rrt_finite(y) && rrt_finite(yaw));
    for (int i = lane; i < 2 * len; i += 64) if (!rrt_finite(path[i])) bad = true;
    if (len < 1 || ballot(bad) != 0ull) {
        if (lane == 0) { A.actions[env] = __builtin_nan(""); A.diag[2 * env] = -1; A.diag[2 * env + 1] = -1; }
        return;
    }
    // nearest waypoint: the first minimum, like np.argmin
    double bd = BP_INF;
    int bi = 0x7FFFFFFF;
    for (int i = lane; i < len; i += 64) {
        const double dx = x - path[2 * i], dy = y - path[2 * i + 1], d2 = dx * dx + dy * dy;
        if (bi == 0x7FFFFFFF || d2 < bd) { bd = d2; bi = i; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double od = __shfl_xor(bd, m);
        const int oi = __shfl_xor(bi, m);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    // `while Lfc > |pos - wp[ind]|: if ind + 1 >= n: break; ind += 1`: the first index from the nearest on that is not within Lfc, or the last
    int ind = len - 1;
    for (int i0 = bi; i0 < len; i0 += 64) {
        const int i = i0 + lane;
        bool stop = false;
        if (i < len) { const double dx = x - path[2 * i], dy = y - path[2 * i + 1]; stop = !(c.Lfc > __builtin_sqrt(dx * dx + dy * dy)); }
        const unsigned long long m = ballot(stop);
        if (m != 0ull) { ind = i0 + (int)__builtin_ctzll(m); break; }
    }
    const double theta_d = bd_atan2(path[2 * ind + 1] - y, path[2 * ind] - x);
    double sn, cs;
    bp_sincos(theta_d - yaw, sn, cs);
    const double theta_e = bd_atan2(sn, cs);
    if (lane == 0) { A.actions[env] = theta_e / c.dt / c.action_scale; A.diag[2 * env] = bi; A.diag[2 * env + 1] = ind; }
}
