// Device-resident replay buffer fed by the ready queue (bp_replay_*; DESIGN.md "Replay buffer").
//
// A ring of C transitions (state, action, reward, ministeps, next_state) plus, per env, the observation the env showed last and the action it was sent for it.
// bp_replay_observe reads the [M, ...] rows of one recv, pairs each transition row with its env's pending observation and action and stores it;
// bp_replay_record notes the actions of one send; bp_replay_sample draws B stored transitions and writes them as float planes.  The caller owns all
// memory; nothing is read back and nothing synchronises.  The bookkeeping kernels are one workgroup that loops over M or B -- exact, not fast -- and decide
// no order with an atomic: a slot is (transitions stored so far + rank of the row among the call's transition rows) % C, the rank from a ballot / LDS scan
// over the rows in ascending order.  The two bandwidth kernels move 16 bytes per lane and access.
//
// The queue holds an env at most once (bp_asyncq.hpp), so an env id occurs at most once among the rows of a recv: observe relies on it -- the thread that
// reads a 16-byte piece of pend_obs[e] for state[slot] is the only one that touches it, and it overwrites it with the piece of obs[j].
#pragma once
#include <hip/hip_runtime.h>

#include "bp_device.hpp"

#define RPL_THREADS 1024
#define RPL_COPY_THREADS 256
#define RPL_HELD 1u       // pend_flags bit 0: pend_obs[e] holds an observation
#define RPL_ACTED 2u      // bit 1: pend_action[e] is the action sent for it
#define RPL_AWAITS 4u     // bit 2: the env was delivered by a recv and awaits its record

struct ReplayBuf {
    int C, E, row16;                  // capacity, envs, 16-byte pieces per observation row
    uint4 *state, *next_state;        // [C][row16]
    int *action;                      // [C]
    float *reward, *ministeps;        // [C]
    unsigned char *nonfinal;          // [C]
    int *env;                         // [C]
    uint4 *pend_obs;                  // [E][row16]
    int *pend_action;                 // [E]
    unsigned char *pend_flags;        // [E]
    long long *hdr;                   // [4] transitions ever stored, sample draws made, dropped transition rows, rejected record rows
    int *row_slot;                    // [max_rows] workspace: the slot of a recv row, -1 = stores nothing
    int *win;                         // [E] workspace: smallest row of a record that names the env
};

struct ReplayBatch {
    float *state, *next_state;        // [B][4][P][P]
    long long *action;                // [B]
    float *reward, *ministeps;        // [B]
    unsigned char *nonfinal;          // [B]
    int *slot;                        // [B]
    unsigned char *valid;             // [B]
};

// Slot index of sample b of draw `draw` among n stored transitions: the high 32 bits of the counter RNG, keyed as bp_rrt_u01 keys its draws, scaled to [0, n).
__host__ __device__ inline long long bp_replay_pick(unsigned long long seed, long long draw, int b, long long n)
{
    const unsigned long long key = bp_splitmix64(seed ^ bp_splitmix64((unsigned long long)draw));
    const unsigned long long z = bp_splitmix64(key ^ (unsigned long long)(unsigned)b);
    return (long long)(((z >> 32) * (unsigned long long)n) >> 32);   // n < 2^31: the product stays below 2^63
}

// Exclusive rank of the rows with f among the block's 1024 rows (ballot in the wave, the 16 wave sums through LDS), and their total.
__device__ __forceinline__ unsigned rpl_rank(const bool f, int *wsum, unsigned &tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    unsigned off = 0;
    tot = 0;
    for (int w = 0; w < RPL_THREADS / 64; w++) {
        const unsigned s = (unsigned)wsum[w];
        if (w < wave) off += s;
        tot += s;
    }
    __syncthreads();   // wsum is written again by the next call
    return off + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}

// Plans one observe: row j with a valid id is a transition row if slices[j] > 0 and its env holds an observation and an action; transition row of rank r
// goes to slot (stored + r) % C.  If more than C arrive, a row whose slot a later row takes again stores nothing (the result of writing them in row order).
// Writes row_slot[M], the slots' scalar columns, the envs' flags and the header.
__global__ __launch_bounds__(RPL_THREADS) void k_replay_plan(const ReplayBuf r, const int *__restrict__ ids, const double *__restrict__ reward,
                                                             const unsigned char *__restrict__ terminated, const double *__restrict__ info,
                                                             const int *__restrict__ slices, const int M, const int ncols, const int mcol)
{
    __shared__ int wsum[RPL_THREADS / 64];
    const int tid = threadIdx.x;
    const unsigned long long stored = (unsigned long long)r.hdr[0];
    unsigned total = 0, dropped = 0;
    for (int j0 = 0; j0 < M; j0 += RPL_THREADS) {       // pass 1: how many transition rows, how many dropped
        const int j = j0 + tid;
        const int e = j < M ? ids[j] : -1;
        const bool tr = e >= 0 && e < r.E && slices[j] > 0;
        const bool has = tr && (r.pend_flags[e] & (RPL_HELD | RPL_ACTED)) == (RPL_HELD | RPL_ACTED);
        unsigned t, d;
        rpl_rank(has, wsum, t);
        rpl_rank(tr && !has, wsum, d);
        total += t;
        dropped += d;
    }
    unsigned base = 0;
    for (int j0 = 0; j0 < M; j0 += RPL_THREADS) {       // pass 2: the slots (the flags are read before this row's thread changes them)
        const int j = j0 + tid;
        const int e = j < M ? ids[j] : -1;
        const bool valid = e >= 0 && e < r.E;
        const bool has = valid && slices[j] > 0 && (r.pend_flags[e] & (RPL_HELD | RPL_ACTED)) == (RPL_HELD | RPL_ACTED);
        unsigned t;
        const unsigned rank = base + rpl_rank(has, wsum, t);
        base += t;
        int slot = -1;
        if (has && total - rank <= (unsigned)r.C) {       // one of the last C transition rows of the call
            slot = (int)((stored + rank) % (unsigned long long)r.C);
            r.action[slot] = r.pend_action[e];
            r.reward[slot] = (float)reward[j];
            r.ministeps[slot] = (float)info[(size_t)j * ncols + mcol];
            r.nonfinal[slot] = terminated[j] != 0 ? 0 : 1;
            r.env[slot] = e;
        }
        if (j < M) r.row_slot[j] = slot;
        if (valid) r.pend_flags[e] = (unsigned char)(RPL_HELD | RPL_AWAITS);
    }
    if (tid == 0) {
        r.hdr[0] = (long long)(stored + total);
        r.hdr[2] += (long long)dropped;
    }
}

// Grid (M, pieces): row j moves its observation.  With a slot: state[slot] <- pend_obs[e], next_state[slot] <- obs[j]; always pend_obs[e] <- obs[j].
__global__ __launch_bounds__(RPL_COPY_THREADS) void k_replay_copy(const ReplayBuf r, const int *__restrict__ ids, const uint4 *__restrict__ obs)
{
    const int j = blockIdx.x;
    const int e = ids[j];
    const int k = blockIdx.y * RPL_COPY_THREADS + threadIdx.x;
    if (e < 0 || e >= r.E || k >= r.row16) return;
    const int slot = r.row_slot[j];
    const uint4 v = obs[(size_t)j * r.row16 + k];
    uint4 *pend = r.pend_obs + (size_t)e * r.row16 + k;
    if (slot >= 0 && slot < r.C) {
        r.state[(size_t)slot * r.row16 + k] = *pend;
        r.next_state[(size_t)slot * r.row16 + k] = v;
    }
    *pend = v;
}

// One record: row j names env ids[j].  Accepted: the env awaits a record and no smaller row names it (the smallest row per env by atomicMin -- a minimum
// does not depend on the order of its operands -- then the apply phase); with reset[j] != 0 the env forgets everything, else it takes the action.
__global__ __launch_bounds__(RPL_THREADS) void k_replay_record(const ReplayBuf r, const double *__restrict__ actions, const int *__restrict__ ids,
                                                               const unsigned char *__restrict__ reset, const int M)
{
    __shared__ int s_rej;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_rej = 0;
    for (int j = tid; j < M; j += RPL_THREADS) {
        const int e = ids[j];
        if (e >= 0 && e < r.E) r.win[e] = 0x7FFFFFFF;
    }
    __syncthreads();
    for (int j = tid; j < M; j += RPL_THREADS) {
        const int e = ids[j];
        if (e >= 0 && e < r.E) atomicMin(&r.win[e], j);
    }
    __syncthreads();
    for (int j0 = 0; j0 < M; j0 += RPL_THREADS) {
        const int j = j0 + tid;
        const int e = j < M ? ids[j] : -1;
        const bool ok = e >= 0 && e < r.E && r.win[e] == j && (r.pend_flags[e] & RPL_AWAITS) != 0;   // (only the winning row reads the byte it changes)
        if (ok) {
            if (reset != nullptr && reset[j] != 0) r.pend_flags[e] = 0;
            else {
                r.pend_action[e] = (int)actions[j];
                r.pend_flags[e] = (unsigned char)((r.pend_flags[e] | RPL_ACTED) & ~RPL_AWAITS);
            }
        }
        const unsigned long long br = __ballot(e >= 0 && !ok);
        if (lane == 0 && br != 0ull) atomicAdd(&s_rej, __popcll(br));   // (a sum: the order of the additions does not matter)
    }
    __syncthreads();
    if (tid == 0) r.hdr[3] += (long long)s_rej;
}

// The slots of one draw and their scalar columns; then the draw counter advances.  n == 0: zeros.
__global__ __launch_bounds__(RPL_THREADS) void k_replay_pick(const ReplayBuf r, const ReplayBatch o, const int B, const unsigned long long seed)
{
    const long long stored = r.hdr[0], draw = r.hdr[1];
    const long long n = stored < (long long)r.C ? stored : (long long)r.C;
    for (int b = threadIdx.x; b < B; b += RPL_THREADS) {
        const bool v = n > 0;
        const int s = v ? (int)bp_replay_pick(seed, draw, b, n) : 0;
        o.slot[b] = s;
        o.valid[b] = v ? 1 : 0;
        o.action[b] = v ? (long long)r.action[s] : 0ll;
        o.reward[b] = v ? r.reward[s] : 0.0f;
        o.ministeps[b] = v ? r.ministeps[s] : 0.0f;
        o.nonfinal[b] = v ? r.nonfinal[s] : (unsigned char)0;
    }
    __syncthreads();
    if (threadIdx.x == 0) r.hdr[1] = draw + 1;
}

// Grid (B, pieces): a lane reads 16 bytes = 4 pixels x 4 channels of state and of next_state and writes one float4 to each of the four planes of both.
// The value of a byte is (float)u8 / 255.0f, an IEEE division, from a 256-entry table the workgroup makes by dividing.
__device__ __forceinline__ void rpl_planes(const uint4 v, const float *tab, float *__restrict__ out, const size_t plane, const int k)
{
    for (int c = 0; c < 4; c++) {
        const int sh = 8 * c;
        const float4 f = make_float4(tab[(v.x >> sh) & 255u], tab[(v.y >> sh) & 255u], tab[(v.z >> sh) & 255u], tab[(v.w >> sh) & 255u]);
        *reinterpret_cast<float4 *>(out + (size_t)c * plane + (size_t)k * 4) = f;
    }
}
__global__ __launch_bounds__(RPL_COPY_THREADS) void k_replay_gather(const ReplayBuf r, const ReplayBatch o)
{
    __shared__ float tab[256];
    tab[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const int b = blockIdx.x;
    const int k = blockIdx.y * RPL_COPY_THREADS + threadIdx.x;
    if (k >= r.row16) return;
    const int s = o.slot[b];
    uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0;
    if (o.valid[b] != 0 && s >= 0 && s < r.C) {
        v0 = r.state[(size_t)s * r.row16 + k];
        v1 = r.next_state[(size_t)s * r.row16 + k];
    }
    const size_t plane = (size_t)r.row16 * 4;           // P * P pixels
    rpl_planes(v0, tab, o.state + (size_t)b * 4 * plane, plane, k);
    rpl_planes(v1, tab, o.next_state + (size_t)b * 4 * plane, plane, k);
}
