// TaskDrivenMetric (benchpush/common/metrics/task_driven_metric.py; host statement: benchpush_amd/metrics/task_driven_metric.py) for box-delivery and
// area-clearing handles, accumulated on the device like ShipIceMetric / MazeNamoMetric are for the other two (k_episode_metrics in bp_capi.hip).
//   tm_area_centroid  shoelace area / centroid of a polygon, sums in vertex order (_area_centroid)
//   tm_mst_cost       Prim over {completed boxes, their goal leaves, robot start}, total summed in the order Prim takes the edges (_mst_weight)
//   tm_row            the six BP_EPM_* columns of one finished episode
//   k_task_metrics    one thread per env after the finish kernels of a step (mode 0) or the reset kernels (mode 1)
// The three functions are __host__ __device__ and plain C++: bp_task_metric_row runs them on the host, so CPU tests exercise the kernel's arithmetic.
// DESIGN.md "Task-driven metrics" states the definition, the tie rule of Prim and the layout of the per-env state.
#pragma once
#include "bp_boxdelivery.hpp"

#define TM_MAXNODE (2 * BD_MAXBOX + 1)

// xy: [n][2] vertices.  out = |a|, cx, cy with a = sum(cross) / 2 and the centroid taken with the signed a.
__host__ __device__ inline void tm_area_centroid(const double *xy, const int n, double *out)
{
    double sa = 0.0, sx = 0.0, sy = 0.0;
    for (int i = 0; i < n; i++) {
        const int j = (i + 1 == n) ? 0 : i + 1;
        const double x = xy[2 * i], y = xy[2 * i + 1], xn = xy[2 * j], yn = xy[2 * j + 1];
        const double cr = x * yn - xn * y;
        sa += cr;
        sx += (x + xn) * cr;
        sy += (y + yn) * cr;
    }
    const double a = sa / 2;
    out[0] = __builtin_fabs(a); out[1] = sx / (6 * a); out[2] = sy / (6 * a);
}

__host__ __device__ inline double tm_norm(const double dx, const double dy) { return __builtin_sqrt(dx * dx + dy * dy); }

// k completed boxes with centroids (cx, cy) and goal distances d, robot start (rx, ry).  Nodes: boxes 0 .. k-1, goal leaf of box i at k + i, robot at 2k.
// Prim from node 0.  The frontier keeps its nodes in the order they entered (boxes 1 .. k-1, robot, goal 0; the goal of a box when that box is taken); among
// equal keys the first one wins, and a key that gets smaller stays where it is -- the iteration order of the host's dict.
__host__ __device__ inline double tm_mst_cost(const int k, const double *cx, const double *cy, const double *d, const double rx, const double ry)
{
    if (k <= 0) return 0.0;
    double key[TM_MAXNODE];
    unsigned char front[TM_MAXNODE];
    int nf = 0;
    const int robot = 2 * k;
    for (int j = 1; j < k; j++) { key[j] = tm_norm(cx[0] - cx[j], cy[0] - cy[j]); front[nf++] = (unsigned char)j; }
    key[robot] = tm_norm(rx - cx[0], ry - cy[0]); front[nf++] = (unsigned char)robot;
    key[k] = d[0]; front[nf++] = (unsigned char)k;
    double total = 0.0;
    while (nf > 0) {
        int at = 0;
        for (int q = 1; q < nf; q++) if (key[front[q]] < key[front[at]]) at = q;
        const int v = front[at];
        total += key[v];
        for (int q = at + 1; q < nf; q++) front[q - 1] = front[q];
        nf--;
        if (v >= k && v != robot) continue;                      // a goal leaf: its only neighbour is taken
        for (int q = 0; q < nf; q++) {                           // min(w, old) of the host: w unless old < w
            const int b = front[q];
            if (b >= k) continue;
            const double w = (v == robot) ? tm_norm(rx - cx[b], ry - cy[b]) : tm_norm(cx[v] - cx[b], cy[v] - cy[b]);
            if (!(key[b] < w)) key[b] = w;
        }
        if (v == robot) continue;
        for (int q = 0; q < nf; q++)
            if (front[q] == robot) { const double w = tm_norm(rx - cx[v], ry - cy[v]); if (!(key[robot] < w)) key[robot] = w; }
        key[k + v] = d[v]; front[nf++] = (unsigned char)(k + v);
    }
    return total;
}

// One finished episode.  boxes: [nbox][3] = area, cx, cy of the polygons at reset; completed: [nbox]; goals: [ngoal][2]; (sx, sy) robot start; l0 the
// robot's path length.  Divisions are IEEE: 0 / 0 and x / 0 give NaN / inf, as the host class does with numpy scalars.
__host__ __device__ inline void tm_row(const int nbox, const double *boxes, const unsigned char *completed, const int ngoal, const double *goals,
                                       const double sx, const double sy, const double m0, const double l0, const double total_work, const double reward,
                                       const double steps, double *out)
{
    double cx[BD_MAXBOX], cy[BD_MAXBOX], d[BD_MAXBOX];
    int k = 0;
    double mmd = 0.0;
    for (int i = 0; i < nbox; i++) {
        if (!completed[i]) continue;
        const double x = boxes[3 * i + 1], y = boxes[3 * i + 2];
        double best = tm_norm(goals[0] - x, goals[1] - y);
        for (int g = 1; g < ngoal; g++) { const double w = tm_norm(goals[2 * g] - x, goals[2 * g + 1] - y); if (w < best) best = w; }
        cx[k] = x; cy[k] = y; d[k] = best; k++;
        mmd += best * boxes[3 * i];
    }
    const double own = m0 * l0;
    out[BP_EPM_EFFICIENCY] = tm_mst_cost(k, cx, cy, d, sx, sy) / l0;
    out[BP_EPM_EFFORT] = (own + mmd) / (own + total_work);
    out[BP_EPM_REWARD] = reward;
    out[BP_EPM_SUCCESS] = (double)k / (double)nbox;
    out[BP_EPM_LENGTH] = steps;
    out[BP_EPM_TOTAL_WORK] = total_work;
}

__device__ __forceinline__ double bp_round2(double x);   // python's round(x, 2) (bp_capi.hip)

// Per-env state of a box handle, all [record]: D.m_acc (layout at the member), the completed flags of the last step in bits 8 .. 31 of D.e_lastflag (the
// reset kernels put Q.alive / Q.cleared back before an episode that a reset closes is emitted), Q.m_box, and D.m_rows / m_ring / m_sum / m_count / m_open
// with the meaning they have for the other environments.  The finish kernels write e_lastrew, bits 0 / 1 of e_lastflag and e_total_work per accepted step.
// mode 0: after the finish kernels of bp_step (ready == nullptr) or of bp_bd_step_async / bp_bd_async_drain (only envs with ready[e] != 0 emitted a
// transition; a busy env's rows are stale by contract).  mode 1: after the reset kernels, envs of the mask.
__global__ __launch_bounds__(256) void k_task_metrics(const DevParams P, const BdParams B, const DevPtrs D, const BdPtrs Q, const int mode,
                                                      const unsigned char *__restrict__ mask, const unsigned char *__restrict__ ready)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= P.num_envs) return;
    double *a = D.m_acc + (size_t)env * 8;
    double *mb = Q.m_box + (size_t)env * BD_MAXBOX * 3;
    const size_t eb = (size_t)env * P.nbcap;
    const d2 p = D.pxy[eb];
    const double x = bp_round2(p.x), y = bp_round2(p.y);
    auto emit = [&]() {
        unsigned char done[BD_MAXBOX];
        const unsigned bits = (unsigned)D.e_lastflag[env] >> 8;
        for (int k = 0; k < BD_MAXBOX; k++) done[k] = (unsigned char)((bits >> k) & 1u);
        const double recept[2] = {B.recept_x, B.recept_y};
        double *r = D.m_rows + (size_t)env * BP_EPM_COUNT;
        tm_row(B.nbox, mb, done, B.task == 1 ? B.ngoal : 1, B.task == 1 ? (const double *)Q.goals : recept, a[4], a[7], B.robot_mass, a[1], a[6], a[0], a[5], r);
        const unsigned n = D.m_count[env];
        double *ring = D.m_ring + ((size_t)env * BP_EPM_RING + n % BP_EPM_RING) * BP_EPM_COUNT, *sum = D.m_sum + (size_t)env * BP_EPM_COUNT;
        for (int q = 0; q < BP_EPM_COUNT; q++) { ring[q] = r[q]; sum[q] += r[q]; }
        D.m_count[env] = n + 1u;
    };
    if (mode == 1) {
        if (mask != nullptr && mask[env] == 0) return;
        if (D.m_open[env] && a[5] > 0.0) emit();   // reset of a running episode: eps_complete by truncation, with the flags of its last step
        const int *nv = D.sc_nv + (size_t)D.e_trial[env] * P.nbcap;
        for (int k = 0; k < BD_MAXBOX; k++) {
            double o[3] = {0.0, 0.0, 0.0};
            if (k < B.nbox) tm_area_centroid((const double *)(D.wv + (eb + B.first_box + k) * BP_MAXV), nv[B.first_box + k], o);
            mb[3 * k] = o[0]; mb[3 * k + 1] = o[1]; mb[3 * k + 2] = o[2];
        }
        a[0] = 0.0; a[1] = 0.0; a[2] = x; a[3] = y; a[4] = x; a[5] = 0.0; a[6] = 0.0; a[7] = y;
        D.e_lastflag[env] = 0;
        D.m_open[env] = 1;
        return;
    }
    if (ready != nullptr && ready[env] == 0) return;   // asynchronous step: the env is still inside its env step (or idle in a drain)
    if (!D.m_open[env]) return;                        // stepped past its end without a reset: nothing to account
    unsigned bits = 0u;
    const unsigned char *flag = (B.task == 1 ? Q.cleared : Q.alive) + (size_t)env * BD_MAXBOX;
    for (int k = 0; k < B.nbox; k++) bits |= (unsigned)((flag[k] != 0) == (B.task == 1)) << k;
    const int fl = D.e_lastflag[env] & 0xFF;
    D.e_lastflag[env] = fl | (int)(bits << 8);
    const double dx = a[2] - x, dy = a[3] - y;
    a[0] += D.e_lastrew[env];
    a[1] += __builtin_sqrt(dx * dx + dy * dy);
    a[2] = x; a[3] = y;
    a[5] += 1.0;
    a[6] = D.e_total_work[env];
    if (fl & 3) { emit(); D.m_open[env] = 0; }
}
