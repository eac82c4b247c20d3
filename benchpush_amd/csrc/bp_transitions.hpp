// Device-resident transition buffer for lock-step envs (bp_transitions_*; DESIGN.md "Transition buffer").
//
// A ring of T step rows of E envs: per add the observation batch the policy acted on, the next observation (the terminal observation where the episode
// ended in this step), the actions, the reward, the done flag and whether the done came from the time limit.  Transition (s, e), s the number of adds
// before it, lives in slot (s % T) * E + e; the number of adds and the number of sample draws are device counters (hdr), so no call reads back and the
// call sequence does not depend on data.  The caller owns all memory; nothing synchronises.  Conventions of bp_replay.hpp and bp_rollout.hpp: the two
// bandwidth kernels move 16 bytes per lane and access; no atomic decides an order; the bookkeeping kernels are one workgroup that loops -- exact, not fast.
//
// All float arithmetic here is binary32 and the build has -ffp-contract=off: a numpy float32 loop in the stated order reproduces the bits.
#pragma once
#include <hip/hip_runtime.h>

#include "bp_device.hpp"
#include "bp_replay.hpp"
#include "bp_rollout.hpp"

#define TRN_MIN_GROUPS 2048     // the bandwidth kernels split a row into more strips than RLO_ROW_STRIPS while rows * strips stays below this

struct TransBuf {
    int T, E, A, row16;               // step rows, envs, action width, 16-byte pieces per observation row
    uint4 *obs, *next_obs;            // [T][E][row16]
    float *action;                    // [T][E][A]
    float *reward;                    // [T][E]
    unsigned char *done, *timeout;    // [T][E]
    long long *hdr;                   // [2] adds ever made, sample draws made
};

struct TransBatch {
    float *obs, *next_obs;            // [B][R]
    float *action;                    // [B][A]
    float *reward, *done;             // [B]
    int *slot;                        // [B]
    unsigned char *valid;             // [B]
};

// add, the rows.  Grid (E, strips): the workgroups of env e move the pieces of obs[e] into the step row's obs and the pieces of terminal_obs[e] (done[e]
// != 0) or next_obs[e] into its next_obs.  The select is a property of the workgroup -- one source pointer, no branch inside a row.  The step row is
// hdr[0] % T, read here and advanced by k_trans_scalars, which the stream orders after this kernel.
__global__ __launch_bounds__(RPL_COPY_THREADS) void k_trans_rows(const TransBuf r, const uint4 *__restrict__ obs, const uint4 *__restrict__ next_obs,
                                                                 const uint4 *__restrict__ terminal_obs, const unsigned char *__restrict__ done)
{
    const int e = blockIdx.x;
    const size_t row = (size_t)(r.hdr[0] % (long long)r.T) * (size_t)r.E + (size_t)e;
    const uint4 *__restrict__ so = obs + (size_t)e * r.row16;
    const uint4 *__restrict__ sn = (done[e] != 0 ? terminal_obs : next_obs) + (size_t)e * r.row16;
    uint4 *__restrict__ d_o = r.obs + row * r.row16;
    uint4 *__restrict__ d_n = r.next_obs + row * r.row16;
    for (int p = blockIdx.y * RPL_COPY_THREADS + threadIdx.x; p < r.row16; p += gridDim.y * RPL_COPY_THREADS) {
        const uint4 a = so[p], b = sn[p];
        d_o[p] = a;
        d_n[p] = b;
    }
}

// add, the scalar columns of step row hdr[0] % T: the E * A actions, reward = (float)reward, done = done != 0, timeout = done && truncated; then, after
// a barrier, hdr[0] += 1 by one thread.
__global__ __launch_bounds__(RPL_THREADS) void k_trans_scalars(const TransBuf r, const float *__restrict__ action, const double *__restrict__ reward,
                                                               const unsigned char *__restrict__ done, const unsigned char *__restrict__ truncated)
{
    const long long adds = r.hdr[0];
    const size_t row = (size_t)(adds % (long long)r.T) * (size_t)r.E;
    const size_t na = (size_t)r.E * (size_t)r.A;
    for (size_t i = threadIdx.x; i < na; i += RPL_THREADS) r.action[row * r.A + i] = action[i];
    for (int e = threadIdx.x; e < r.E; e += RPL_THREADS) {
        const bool d = done[e] != 0;
        r.reward[row + e] = (float)reward[e];
        r.done[row + e] = d ? 1 : 0;
        r.timeout[row + e] = (d && truncated[e] != 0) ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) r.hdr[0] = adds + 1;
}

// sample, the index step: n = min(hdr[0], T) * E stored transitions, sample b reads slot bp_replay_pick(seed, hdr[1], b, n); writes slot, valid and the
// scalar columns, done = done * (1 - timeout) in float; then the draw counter advances.  n == 0: zeros, slot -1.
__global__ __launch_bounds__(RPL_THREADS) void k_trans_pick(const TransBuf r, const TransBatch o, const int B, const unsigned long long seed)
{
    const long long adds = r.hdr[0], draw = r.hdr[1];
    const long long n = (adds < (long long)r.T ? adds : (long long)r.T) * (long long)r.E;
    for (int b = threadIdx.x; b < B; b += RPL_THREADS) {
        const bool v = n > 0;
        const int s = v ? (int)bp_replay_pick(seed, draw, b, n) : -1;
        o.slot[b] = s;
        o.valid[b] = v ? 1 : 0;
        o.reward[b] = v ? r.reward[s] : 0.0f;
        const float d = (v && r.done[s] != 0) ? 1.0f : 0.0f, t = (v && r.timeout[s] != 0) ? 1.0f : 0.0f;
        o.done[b] = d * (1.0f - t);
        for (int a = 0; a < r.A; a++) o.action[(size_t)b * r.A + a] = v ? r.action[(size_t)s * r.A + a] : 0.0f;
    }
    __syncthreads();
    if (threadIdx.x == 0) r.hdr[1] = draw + 1;
}

// sample, the rows.  Grid (B, strips, 2): plane 0 writes row slot[b] of obs, plane 1 of next_obs, as floats (rlo_float_row: (float)u8 / 255.0f from
// the divide table, 16 bytes read and four float4 written per lane and turn).  Zeros for valid[b] == 0 or a slot outside [0, T * E).
__global__ __launch_bounds__(RPL_COPY_THREADS) void k_trans_gather(const TransBuf r, const TransBatch o)
{
    __shared__ float tab[256];
    rlo_u8_table(tab);
    const int b = blockIdx.x;
    const long long s = (long long)o.slot[b];
    const bool ok = o.valid[b] != 0 && s >= 0 && s < (long long)r.T * r.E;
    const bool nx = blockIdx.z != 0;
    rlo_float_row(tab, nx ? r.next_obs : r.obs, s, ok, r.row16, nx ? o.next_obs : o.obs, b, (int)blockIdx.y, (int)gridDim.y);
}
