// Device-resident ready queue of the asynchronous step of box-delivery / area-clearing (bp_bd_queue_*; DESIGN.md "Asynchronous step").
//
// A FIFO ring of env ids with capacity E between the slice call and the policy: bp_bd_queue_recv appends the envs that emitted a transition, pops up to M ids
// and gathers their rows into dense [M, ...] outputs; bp_bd_queue_send scatters the actions of those ids back and lets the envs start.  An env is in the ring
// at most once, so the ring cannot overflow.  Nothing here decides an order with an atomic: the ring order is (enqueue event, env id), and the events are the
// launches of one stream.  Every kernel but the gather is one workgroup that loops over E or M -- a few KB of work that has to be exact, not fast.
#pragma once
#include <hip/hip_runtime.h>

#define BDQ_THREADS 1024
#define BDQ_HELD 3            // group byte Q.unfin of a held env: it emitted a transition or was reset and waits in the ring or for its send
#define BDQ_GATHER_THREADS 256

struct BdQueue {
    int *ring;                // [E] env ids, FIFO from hdr[0]
    int *hdr;                 // [4] head, ids queued, rejected send rows so far, -
    unsigned char *where;     // [E] 0 = not in the queue's hands (idle / busy), 1 = in the ring, 2 = taken by a recv and awaiting its send
    unsigned char *fresh;     // [E] 1 = the env's queued row is a reset observation (no transition: reward 0, flags 0, slices 0)
    unsigned char *rmask;     // [E] envs that the last send resets (mask of the masked reset that follows it)
    int *win;                 // [E] smallest row of a send that names the env
    double *actions;          // [E][action_dim] the envs' action rows (k_bd_plan_async reads them when an idle env starts)
};

// Ordered stream compaction of a byte mask into the ring: the envs with mask[e] != 0 (mask == nullptr: every env) that the queue does not hold yet are appended
// in ascending env id and become held.  In-wave rank from the ballot, wave offsets from a scan over the 16 wave sums in LDS, chunk after chunk.
__global__ __launch_bounds__(BDQ_THREADS) void k_bdq_enqueue(const BdQueue q, unsigned char *__restrict__ unfin, const unsigned char *__restrict__ mask,
                                                             const int E, const int fresh)
{
    __shared__ int wsum[BDQ_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned head = (unsigned)q.hdr[0], queued = (unsigned)q.hdr[1];
    unsigned base = 0;
    for (int e0 = 0; e0 < E; e0 += BDQ_THREADS) {
        const int e = e0 + tid;
        const bool f = e < E && (mask == nullptr || mask[e] != 0) && q.where[e] == 0;
        const unsigned long long b = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        unsigned off = 0, tot = 0;
        for (int w = 0; w < BDQ_THREADS / 64; w++) {
            const unsigned s = (unsigned)wsum[w];
            if (w < wave) off += s;
            tot += s;
        }
        if (f) {
            const unsigned rank = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
            q.ring[(head + queued + base + off + rank) % (unsigned)E] = e;
            unfin[e] = BDQ_HELD;
            q.where[e] = 1;
            q.fresh[e] = (unsigned char)fresh;
        }
        base += tot;
        __syncthreads();   // wsum is written again by the next chunk
    }
    if (tid == 0) q.hdr[1] = (int)(queued + base);
}

// Pops up to M ids from the head into ids[M] (rows beyond the count: -1), marks them taken and writes the counts of the call:
// counts[0] rows delivered, [1] still queued, [2] busy envs, [3] envs taken and not sent yet (these rows included), [4] rejected send rows so far.
// full_only != 0: nothing is taken while fewer than M ids are queued and an env is still busy (the blocking recv repeats the call until a batch is delivered).
__global__ __launch_bounds__(BDQ_THREADS) void k_bdq_take(const BdQueue q, const unsigned char *__restrict__ unfin, const int E, const int M,
                                                          const int full_only, int *__restrict__ ids, int *__restrict__ counts)
{
    __shared__ int s_busy, s_taken;
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned head = (unsigned)q.hdr[0];
    const int queued = q.hdr[1], rejected = q.hdr[2];
    if (tid == 0) { s_busy = 0; s_taken = 0; }
    __syncthreads();
    for (int e0 = 0; e0 < E; e0 += BDQ_THREADS) {
        const int e = e0 + tid;
        const unsigned long long bb = __ballot(e < E && unfin[e] == 1);
        const unsigned long long bt = __ballot(e < E && q.where[e] == 2);
        if (lane == 0) { atomicAdd(&s_busy, __popcll(bb)); atomicAdd(&s_taken, __popcll(bt)); }   // (sums: the order of the additions does not matter)
    }
    __syncthreads();
    const int busy = s_busy;
    const int n = (full_only != 0 && queued < M && busy > 0) ? 0 : min(M, min(queued, E));
    for (int j = tid; j < M; j += BDQ_THREADS) {
        int id = -1;
        if (j < n) {
            id = q.ring[(head + (unsigned)j) % (unsigned)E];
            q.where[id] = 2;
        }
        ids[j] = id;
    }
    if (tid == 0) {
        q.hdr[0] = (int)((head + (unsigned)n) % (unsigned)E);
        q.hdr[1] = queued - n;
        counts[0] = n; counts[1] = queued - n; counts[2] = busy; counts[3] = s_taken + n; counts[4] = rejected;
    }
}

// Row j of the dense outputs gets the rows of env ids[j]; a row with id -1 stores zeros and reads nothing.  Grid (tiles, M): a workgroup reads its id once and
// every lane moves 16 B of the observation row per load / store; reward, flags, info and slices ride in the first tile's workgroup.
__global__ __launch_bounds__(BDQ_GATHER_THREADS) void k_bdq_gather(const int *__restrict__ ids, const unsigned char *__restrict__ fresh, const int E,
                                                                   const uint4 *__restrict__ obs_e, uint4 *__restrict__ obs_m, const int row16,
                                                                   const double *__restrict__ rew_e, const unsigned char *__restrict__ term_e,
                                                                   const unsigned char *__restrict__ trunc_e, const double *__restrict__ info_e,
                                                                   const int *__restrict__ slices_e, double *__restrict__ rew_m,
                                                                   unsigned char *__restrict__ term_m, unsigned char *__restrict__ trunc_m,
                                                                   double *__restrict__ info_m, int *__restrict__ slices_m, const int ncols)
{
    const int j = blockIdx.y;
    const int id = ids[j];
    const bool valid = id >= 0 && id < E;
    const int k = blockIdx.x * BDQ_GATHER_THREADS + threadIdx.x;
    if (obs_m != nullptr && k < row16) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (valid) v = obs_e[(size_t)id * row16 + k];
        obs_m[(size_t)j * row16 + k] = v;
    }
    if (blockIdx.x == 0) {
        const bool trans = valid && fresh[id] == 0;   // a fresh row carries the reset observation and info only
        for (int c = threadIdx.x; c < ncols; c += BDQ_GATHER_THREADS) info_m[(size_t)j * ncols + c] = valid ? info_e[(size_t)id * ncols + c] : 0.0;
        if (threadIdx.x == 0) {
            rew_m[j] = trans ? rew_e[id] : 0.0;
            term_m[j] = trans ? term_e[id] : (unsigned char)0;
            trunc_m[j] = trans ? trunc_e[id] : (unsigned char)0;
            slices_m[j] = trans ? slices_e[id] : 0;
        }
    }
}

// One send: row j names env ids[j].  A row is accepted if its env is taken and awaiting its send and no smaller row names the same env (atomicMin of j per env,
// then the apply phase: the outcome does not depend on which thread runs first); ids[j] == -1 is ignored; every other row is rejected and counted.  An accepted
// row either hands the env its action (the env is idle and starts in the next recv) or, with reset[j] != 0, puts it into the mask of the masked reset that the
// host enqueues next (the env stays held; k_bdq_enqueue appends it as a fresh row after that reset).
__global__ __launch_bounds__(BDQ_THREADS) void k_bdq_send(const BdQueue q, unsigned char *__restrict__ unfin, const int E, const int M, const int adim,
                                                          const double *__restrict__ actions, const int *__restrict__ ids,
                                                          const unsigned char *__restrict__ reset)
{
    __shared__ int s_rej;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_rej = 0;
    for (int e = tid; e < E; e += BDQ_THREADS) q.rmask[e] = 0;
    for (int j = tid; j < M; j += BDQ_THREADS) {
        const int id = ids[j];
        if (id >= 0 && id < E) q.win[id] = 0x7FFFFFFF;
    }
    __syncthreads();
    for (int j = tid; j < M; j += BDQ_THREADS) {
        const int id = ids[j];
        if (id >= 0 && id < E) atomicMin(&q.win[id], j);
    }
    __syncthreads();
    for (int j0 = 0; j0 < M; j0 += BDQ_THREADS) {
        const int j = j0 + tid;
        const int id = j < M ? ids[j] : -1;
        const bool named = id != -1;
        const bool ok = id >= 0 && id < E && q.win[id] == j && q.where[id] == 2;   // (only the winning row reads the state byte it is about to change)
        if (ok) {
            q.where[id] = 0;
            if (reset != nullptr && reset[j] != 0) q.rmask[id] = 1;
            else {
                for (int a = 0; a < adim; a++) q.actions[(size_t)id * adim + a] = actions[(size_t)j * adim + a];
                unfin[id] = 0;
            }
        }
        const unsigned long long br = __ballot(named && !ok);
        if (lane == 0 && br != 0ull) atomicAdd(&s_rej, __popcll(br));
    }
    __syncthreads();
    if (tid == 0) q.hdr[2] += s_rej;
}
