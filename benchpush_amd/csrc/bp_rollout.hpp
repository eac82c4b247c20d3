// Device-resident on-policy rollout buffer with GAE (bp_rollout_*; DESIGN.md "Rollout buffer").
//
// T steps of E envs: per step the observation batch the policy acted on ([E][R] bytes), its actions, values and log-probabilities, the reward and the
// episode-start flags; then advantages and returns by a backward scan, and shuffled minibatches as float rows.  The step index, the epoch and the minibatch
// number are host integers -- the call sequence does not depend on data.  The caller owns all memory; nothing is read back and nothing synchronises.
// Conventions of bp_replay.hpp: the bandwidth kernels move 16 bytes per lane and access; the rank of a masked env comes from a ballot / LDS scan over the
// envs in ascending order (rpl_rank), never from an atomic; the bookkeeping kernels are one workgroup that loops -- exact, not fast.
//
// All float arithmetic here is binary32 and the build has -ffp-contract=off: a numpy float32 loop in the stated order reproduces the bits.
#pragma once
#include <hip/hip_runtime.h>

#include "bp_device.hpp"
#include "bp_replay.hpp"

#define RLO_COPY_BLOCKS 4096    // the copy of begin strides beyond this many workgroups
#define RLO_ROW_STRIPS 8        // workgroups per row of the float gather at most
#define RLO_GAE_THREADS 64      // one wave per workgroup: the scan is latency bound, so the envs are spread over as many CUs as there are waves

struct RolloutBuf {
    int T, E, A, row16;               // steps, envs, action width, 16-byte pieces per observation row
    uint4 *obs;                       // [T][E][row16]
    float *action;                    // [T][E][A]
    float *reward, *value, *logp, *advantage, *ret;   // [T][E]
    unsigned char *episode_start;     // [T][E]
    unsigned char *last_done;         // [E]
    long long *hdr;                   // [2] truncated rows left without a bootstrap, rows stored
};

struct RolloutBatch {
    float *obs;                       // [B][R]
    float *action;                    // [B][A]
    float *value, *logp, *advantage, *ret;   // [B]
    int *index;                       // [B]
    unsigned char *valid;             // [B]
};

// Keyed bijection of [0, n), 1 <= n < 2^31: a 4-round balanced Feistel network over 2h bits, h the smallest value with 4^h >= n, walked until the value
// is below n (the network permutes the 2h-bit domain, so the walk returns to [0, n)).  Round r maps (left, right) to (right, left ^ F_r(right)) with
// F_r(right) = low h bits of bp_splitmix64(key ^ (r << 32 | right)) >> 32.
__host__ __device__ inline long long bp_rollout_perm(unsigned long long seed, long long epoch, long long i, long long n)
{
    int h = 0;
    while ((1ll << (2 * h)) < n) h++;
    const unsigned long long mask = (1ull << h) - 1ull;
    const unsigned long long key = bp_splitmix64(seed ^ bp_splitmix64((unsigned long long)epoch));
    unsigned long long x = (unsigned long long)i;
    do {
        unsigned long long left = x >> h, right = x & mask;
        for (unsigned long long r = 0; r < 4; r++) {
            const unsigned long long f = (bp_splitmix64(key ^ ((r << 32) | right)) >> 32) & mask;
            const unsigned long long nr = left ^ f;
            left = right;
            right = nr;
        }
        x = (left << h) | right;
    } while (x >= (unsigned long long)n);
    return (long long)x;
}

// begin: the threads stride over the pieces of the [E][row16] observation batch and move them into obs[t]; the same stride stores the E * A actions and
// the E values, log-probabilities and episode_start[t] = last_done.
__global__ __launch_bounds__(RPL_COPY_THREADS) void k_rollout_begin(const RolloutBuf r, const int t, const uint4 *__restrict__ obs,
                                                                    const float *__restrict__ action, const float *__restrict__ value,
                                                                    const float *__restrict__ logp)
{
    const size_t first = (size_t)blockIdx.x * RPL_COPY_THREADS + threadIdx.x, stride = (size_t)gridDim.x * RPL_COPY_THREADS;
    const size_t pieces = (size_t)r.E * (size_t)r.row16, na = (size_t)r.E * (size_t)r.A;
    uint4 *dst = r.obs + (size_t)t * pieces;
    for (size_t i = first; i < pieces; i += stride) dst[i] = obs[i];
    for (size_t i = first; i < na; i += stride) r.action[(size_t)t * na + i] = action[i];
    for (size_t i = first; i < (size_t)r.E; i += stride) {
        const size_t c = (size_t)t * r.E + i;
        r.value[c] = value[i];
        r.logp[c] = logp[i];
        r.episode_start[c] = r.last_done[i] != 0 ? 1 : 0;
    }
}

// pick: the first K envs with mask[e] != 0 in ascending order; out_ids[k] = e, -1 beyond the number found; hdr[0] += masked envs beyond K.
__global__ __launch_bounds__(RPL_THREADS) void k_rollout_pick(const RolloutBuf r, const unsigned char *__restrict__ mask, const int K,
                                                              int *__restrict__ out_ids)
{
    __shared__ int wsum[RPL_THREADS / 64];
    const int tid = threadIdx.x;
    unsigned base = 0;
    for (int e0 = 0; e0 < r.E; e0 += RPL_THREADS) {
        const int e = e0 + tid;
        const bool f = e < r.E && mask[e] != 0;
        unsigned tot;
        const unsigned rank = base + rpl_rank(f, wsum, tot);
        base += tot;
        if (f && rank < (unsigned)K) out_ids[rank] = e;
    }
    for (unsigned k = base + (unsigned)tid; k < (unsigned)K; k += RPL_THREADS) out_ids[k] = -1;   // (ranks below `base` were written above)
    if (tid == 0 && base > (unsigned)K) r.hdr[0] += (long long)(base - (unsigned)K);
}

// The 256-entry table tab[u] = (float)u / 255.0f, an IEEE division, made by the 256 threads of a workgroup (RPL_COPY_THREADS) by dividing.
__device__ __forceinline__ void rlo_u8_table(float *tab)
{
    tab[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
}

// Row `s` of `src` as floats into row `k` of `out`, this workgroup's share: the row's pieces are dealt to `strips` workgroups in turns of 256, a lane reads
// 16 bytes and writes four float4 per turn.  Zeros where !ok (workgroup-uniform; nothing is read then).
__device__ __forceinline__ void rlo_float_row(const float *tab, const uint4 *__restrict__ src, const long long s, const bool ok, const int row16,
                                              float *__restrict__ out, const int k, const int strip, const int strips)
{
    for (int p = strip * RPL_COPY_THREADS + threadIdx.x; p < row16; p += strips * RPL_COPY_THREADS) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (ok) v = src[(size_t)s * row16 + p];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        float4 *o = reinterpret_cast<float4 *>(out + ((size_t)k * row16 + p) * 16);
        for (int c = 0; c < 4; c++)
            o[c] = ok ? make_float4(tab[w[c] & 255u], tab[(w[c] >> 8) & 255u], tab[(w[c] >> 16) & 255u], tab[(w[c] >> 24) & 255u])
                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// Grid (rows, strips): row k of `out` is row ids[k] of `src` as floats, (float)u8 / 255.0f by IEEE division from a 256-entry table the workgroup makes by
// dividing; a lane reads 16 bytes and writes four float4 per turn, the row's pieces dealt to the strips in turns of 256.  Zeros for ids[k] outside
// [0, limit) or valid[k] == 0 (valid may be NULL).
__global__ __launch_bounds__(RPL_COPY_THREADS) void k_rollout_rows(const uint4 *__restrict__ src, const int *__restrict__ ids,
                                                                   const unsigned char *__restrict__ valid, const long long limit, const int row16,
                                                                   float *__restrict__ out)
{
    __shared__ float tab[256];
    rlo_u8_table(tab);
    const int k = blockIdx.x;
    const long long s = (long long)ids[k];
    const bool ok = s >= 0 && s < limit && (valid == nullptr || valid[k] != 0);
    rlo_float_row(tab, src, s, ok, row16, out, k, (int)blockIdx.y, (int)gridDim.y);
}

// end: reward[t][e] = (float)reward[e] and last_done = done for every env; then, after a barrier, the bootstrap rows: reward[t][e] += g * boot_values[k]
// for boot_ids[k] = e in [0, E) (the ids >= 0 of one call are distinct, as bp_rollout_pick_rows makes them).  hdr[1] += E.
__global__ __launch_bounds__(RPL_THREADS) void k_rollout_end(const RolloutBuf r, const int t, const double *__restrict__ reward,
                                                             const unsigned char *__restrict__ done, const int *__restrict__ boot_ids,
                                                             const float *__restrict__ boot_values, const int K, const float g)
{
    float *row = r.reward + (size_t)t * r.E;
    for (int e = threadIdx.x; e < r.E; e += RPL_THREADS) {
        row[e] = (float)reward[e];
        r.last_done[e] = done[e] != 0 ? 1 : 0;
    }
    __syncthreads();
    if (boot_ids != nullptr)
        for (int k = threadIdx.x; k < K; k += RPL_THREADS) {
            const int e = boot_ids[k];
            if (e >= 0 && e < r.E) row[e] = row[e] + g * boot_values[k];
        }
    if (threadIdx.x == 0) r.hdr[1] += (long long)r.E;
}

// finish: one lane per env scans t = T-1 .. 0; lanes of a wave read consecutive envs of a [T][E] row.
__global__ __launch_bounds__(RLO_GAE_THREADS) void k_rollout_gae(const RolloutBuf r, const float *__restrict__ last_values, const float g, const float gl)
{
    const int e = blockIdx.x * RLO_GAE_THREADS + threadIdx.x;
    if (e >= r.E) return;
    float v_next = last_values[e];
    float nn = 1.0f - (r.last_done[e] != 0 ? 1.0f : 0.0f);
    float adv = 0.0f;
    for (int t = r.T - 1; t >= 0; t--) {
        const size_t c = (size_t)t * r.E + e;
        const float v = r.value[c];
        const float delta = (r.reward[c] + (g * v_next) * nn) - v;
        adv = delta + (gl * nn) * adv;
        r.advantage[c] = adv;
        r.ret[c] = adv + v;
        v_next = v;
        nn = 1.0f - (r.episode_start[c] != 0 ? 1.0f : 0.0f);
    }
}

// minibatch, the index step: sample b of minibatch j is position pos = j * B + b of the epoch's permutation; valid = pos < N.  Writes index, valid and the
// scalar columns (zeros for a sample that is not valid).
__global__ __launch_bounds__(RPL_COPY_THREADS) void k_rollout_index(const RolloutBuf r, const RolloutBatch o, const unsigned long long seed,
                                                                    const long long epoch, const long long first, const int B)
{
    const int b = blockIdx.x * RPL_COPY_THREADS + threadIdx.x;
    if (b >= B) return;
    const long long N = (long long)r.T * r.E, pos = first + b;
    const bool v = pos < N;
    const long long i = v ? bp_rollout_perm(seed, epoch, pos, N) : 0;
    o.index[b] = (int)i;
    o.valid[b] = v ? 1 : 0;
    o.value[b] = v ? r.value[i] : 0.0f;
    o.logp[b] = v ? r.logp[i] : 0.0f;
    o.advantage[b] = v ? r.advantage[i] : 0.0f;
    o.ret[b] = v ? r.ret[i] : 0.0f;
    for (int a = 0; a < r.A; a++) o.action[(size_t)b * r.A + a] = v ? r.action[(size_t)i * r.A + a] : 0.0f;
}
