// Path tracking (bp_track_path): the controller of the reference's planning-based ship-ice policy (PlanningBasedPolicy.act,
// baselines/ship_ice_nav/planning_based/policy.py:61-172) for every env in one launch.  DESIGN.md ("Path tracking") states the semantics;
// tests/track_ref.py restates them in scalar Python.
//
// One wavefront (= one workgroup of 64 threads) per env.
//   1. The lanes scan the counted samples and the pose for a non-finite component.
//   2. Each lane keeps the smallest (d2, index) of its samples i = lane, lane + 64, ...; a butterfly over the lanes leaves the smallest key in all of
//      them: the smallest index of the minimum, like np.argmin.
//   3. A walk along the path (trk_walk) takes 64 segments per chunk: the lanes compute one segment length each, then the running distance is summed in
//      lane order, starting from +0.0 and testing `dist < limit` before every add, exactly like the reference's while loop.  All lanes hold the same
//      running distance, so every branch is wave-uniform.
//   4. The controller's scalar arithmetic is done by all lanes alike (deterministic bd_atan2 / bp_sincos, no contraction); lane 0 stores.
// Every loop is bounded by P; there are no atomics, no LDS and no waits.  Plain vector loads and stores only.
#pragma once
#include "bp_boxdelivery.hpp"   // bd_atan2

struct TrackArgs {
    bp_track_config c;
    long long path_stride;           // doubles between the envs' paths (0: one path for all)
    const double *paths, *poses;
    const int *lengths;
    const unsigned char *active;
    double *state, *actions, *ct_err;
    int *diag;
};

__device__ __forceinline__ bool trk_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ double trk_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }   // np.clip for a finite v, lo <= hi

// `dist, j = 0.0, start; while dist < limit and <a next sample exists>: dist += |p[next] - p[j]|; j = next` with next = j + dir (dir = +1 or -1) over
// the samples 0 .. len-1.  Returns j (wave-uniform).  At most ceil(len / 64) chunks.
__device__ __forceinline__ int trk_walk(const double *path, int start, int dir, double limit, int len, int lane)
{
    int j = start;
    double dist = 0.0;
    for (;;) {
        const int left = dir > 0 ? len - 1 - j : j;     // segments between j and the end of the path in walk order
        if (!(dist < limit) || left <= 0) break;
        const int n = min(64, left);
        double seg = 0.0;
        if (lane < n) {
            const int a = j + dir * lane;               // forward: samples (a, a + 1); backward: (a, a - 1)
            const int hi = dir > 0 ? a + 1 : a, lo = hi - 1;
            const double ddx = path[3 * hi] - path[3 * lo], ddy = path[3 * hi + 1] - path[3 * lo + 1];
            seg = __builtin_sqrt(ddx * ddx + ddy * ddy);
        }
        int l = 0;
        for (; l < n; l++) {
            if (!(dist < limit)) break;
            dist += __shfl(seg, l);
        }
        j += dir * l;
        if (l < n) break;
    }
    return j;
}

__global__ __launch_bounds__(64) void k_track_path(const TrackArgs A)
{
    const int lane = (int)threadIdx.x;
    const size_t env = blockIdx.x;
    if (A.active && !A.active[env]) return;
    int len = A.c.P;
    if (A.lengths) len = min(A.lengths[env], A.c.P);
    if (len < 1) return;
    const bp_track_config &c = A.c;
    const double *path = A.paths + env * (size_t)A.path_stride;
    const double sx = A.poses[3 * env], sy = A.poses[3 * env + 1], syaw = A.poses[3 * env + 2];
    bool bad = !(trk_finite(sx) && trk_finite(sy) && trk_finite(syaw));
    for (int i = lane; i < 3 * len; i += 64) if (!trk_finite(path[i])) bad = true;
    if (ballot(bad) != 0ull) {
        if (lane == 0) {
            const double nan = __builtin_nan("");
            A.actions[2 * env] = nan; A.actions[2 * env + 1] = nan; A.ct_err[env] = nan;
            if (A.diag) { A.diag[4 * env] = -1; A.diag[4 * env + 1] = 0; A.diag[4 * env + 2] = -1; A.diag[4 * env + 3] = -1; }
        }
        return;
    }
    // nearest sample: the smallest index of the minimum of d2
    double bd = BP_INF;
    int bi = 0x7FFFFFFF;
    for (int i = lane; i < len; i += 64) {
        const double dx = path[3 * i] - sx, dy = path[3 * i + 1] - sy;
        const double d2 = dx * dx + dy * dy;
        if (bi == 0x7FFFFFFF || d2 < bd) { bd = d2; bi = i; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double od = __shfl_xor(bd, m);
        const int oi = __shfl_xor(bi, m);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    const int i_near = bi;
    const double ct = __builtin_sqrt(bd);
    const double xn = path[3 * i_near], yn = path[3 * i_near + 1];
    const int k = trk_walk(path, i_near, -1, c.d_back, len, lane);
    const int j2 = trk_walk(path, i_near, +1, c.d_ahead, len, lane);
    double int_yaw = A.state[4 * env], prev_yaw = A.state[4 * env + 1], int_v = A.state[4 * env + 2], has_yaw = A.state[4 * env + 3];
    double omega, sn, cs;
    int branch, jt;
    if (ct > c.thresh) {
        jt = trk_walk(path, i_near, +1, c.look_car, len, lane);
        const double yaw_ref = bd_atan2(path[3 * jt + 1] - sy, path[3 * jt] - sx);
        bp_sincos(yaw_ref - syaw, sn, cs);
        const double yaw_err = bd_atan2(sn, cs);
        const double vbx = xn - path[3 * k], vby = yn - path[3 * k + 1];
        const double vfx = path[3 * j2] - xn, vfy = path[3 * j2 + 1] - yn;
        const double ang_seg = __builtin_fabs(bd_atan2(vbx * vfy - vby * vfx, vbx * vfx + vby * vfy));
        if (ang_seg < c.straight_ang && __builtin_fabs(yaw_err) > c.yaw_big) {
            branch = 1;
            omega = (yaw_err > 0.0 ? 1.0 : (yaw_err < 0.0 ? -1.0 : 0.0)) * c.omega_small;
        } else {
            branch = 2;
            if (has_yaw == 0.0) { int_yaw = 0.0; prev_yaw = yaw_err; has_yaw = 1.0; }
            if (__builtin_fabs(yaw_err) > c.dead) int_yaw = trk_clip(int_yaw + yaw_err * c.dt, -c.i_cap, c.i_cap);
            else int_yaw = int_yaw * 0.8;
            const double d_yaw = (yaw_err - prev_yaw) / c.dt;
            prev_yaw = yaw_err;
            omega = trk_clip(c.kp * yaw_err + c.ki * int_yaw + c.kd * d_yaw, -c.omega_max, c.omega_max);
        }
    } else {
        branch = 3;
        jt = j2;
        const double yaw_ref = bd_atan2(path[3 * j2 + 1] - path[3 * k + 1], path[3 * j2] - path[3 * k]);
        bp_sincos(yaw_ref - syaw, sn, cs);
        const double yaw_err = bd_atan2(sn, cs);
        omega = trk_clip(yaw_err / c.dt, -c.omega_max, c.omega_max);
    }
    int_v = trk_clip(int_v + c.ki_v * ct * c.dt, 0.0, c.v_max);
    const double pv = c.kp_v * ct + int_v;
    const double v_cmd = pv < c.v_max ? pv : c.v_max;
    if (lane == 0) {
        A.actions[2 * env] = omega / c.action_scale; A.actions[2 * env + 1] = 20.0 * v_cmd; A.ct_err[env] = ct;
        A.state[4 * env] = int_yaw; A.state[4 * env + 1] = prev_yaw; A.state[4 * env + 2] = int_v; A.state[4 * env + 3] = has_yaw;
        if (A.diag) { A.diag[4 * env] = i_near; A.diag[4 * env + 1] = branch; A.diag[4 * env + 2] = jt; A.diag[4 * env + 3] = k; }
    }
}
