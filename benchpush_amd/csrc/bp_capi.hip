// libbenchpush_hip.so: C ABI (include/benchpush_amd.h) over the gfx950 kernels.  No torch types, no CPU fallback:
// every entry point fails with BP_ENODEVICE / BP_EHIP when the GPU path cannot run.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include "bp_host_scene.hpp"
#include "bp_boxdelivery.hpp"
#include "bp_policy.hpp"
#include "bp_render.hpp"
#include "bp_state.hpp"
#include "bp_swath.hpp"
#include "bp_lattice.hpp"
#include "bp_track.hpp"
#include "bp_rrt.hpp"
#include "bp_gtsp.hpp"
#include "bp_asyncq.hpp"
#include "bp_replay.hpp"
#include "bp_rollout.hpp"
#include "bp_transitions.hpp"

// The kernels of a ship-ice / maze handle, one per role, chosen once at load (rigid_kernels): the 8-vertex maze instantiations, the generic pair of a
// handle with damping (no scheduler), or the ship-ice ones.
typedef void (*StepKernel)(const DevParams, const DevPtrs, const double *, double *, unsigned char *, unsigned char *, double *);
typedef void (*ResidentKernel)(const DevParams *, const DevPtrs *, const double *, double *, unsigned char *, unsigned char *, double *);
typedef void (*ResetKernel)(const DevParams, const DevPtrs, const unsigned char *, double *, const int);
struct RigidKernels {
    StepKernel step = nullptr;          // one workgroup per env
    StepKernel sched = nullptr;         // dispatcher-driven scheduled launch, and its completion launch
    ResidentKernel resident = nullptr;  // scheduled launch on resident wavefronts (of a pairing launch: k_physics_step_schedr)
    ResetKernel reset = nullptr;        // settles the templates at load, re-settles in reset() (bp_handle::resettle)
};

struct bp_handle {
    bp_config cfg;
    int num_envs = 0;
    long long env_offset = 0;
    int device = 0;
    int nbcap = 0;
    int num_trials = 0;
    bool loaded = false, was_reset = false;
    int *order_buf = nullptr;
    bool steps_done = false;
    bool resettle = false; // true: reset() re-runs the settle sub-steps instead of copying the settled template
    bool damp = false;     // bp_config.damping_pow != 0: k_physics_step_damp / k_physics_reset_damp (generic vertex loops, no scheduler)
    RigidKernels k;                 // ship-ice / maze: the kernel of each role
    BpLaunchPolicy pol = {};        // ship-ice / maze: the load-time policy of (num_envs, num_cus), bp_policy.hpp; the BP_* variables override its fields in the loader
    int pair_mode = 0;              // two envs per wavefront (bp_physics_pair.hpp): 1 = fixed pairs for the whole step (k_physics_step_pair), 2 = inside the scheduler
    int pair_resident = 0;          // > 0: pairing launches run k_physics_step_schedr with this many resident workgroups (BP_PAIR_RESIDENT)
    int sched_persist = 0;          // > 0: the scheduled launch is k_physics_step_schedl with this many resident workgroups (BP_SCHED_PERSIST)
    void *pd_buf = nullptr;         // its launch constants in device memory (DevParams, DevPtrs)
    int sched_chunk = 0;            // > 0: k_physics_step_sched (preemptive scheduler, chunks of this many sub-steps) is the step kernel; BP_SCHED=0 turns it off
    std::string dev_lock_key;       // non-empty: this handle holds a share of the per-device residency lock (resident_* below)
    bool resident_auto = false;     // resident launches fall back to dispatcher-driven ones while another PROCESS uses the device (checked every few launches)
    bool device_shared = false;     // result of the last check
    unsigned launches = 0;
    int num_cus = 0;                // multiProcessorCount of the handle's device
    hipStream_t st_aux = nullptr;   // box-delivery / area-clearing: the robot's spfa map runs beside the finish kernel; ship-ice: the solo kernel of a pairing launch
    hipStream_t st_aux2 = nullptr;  // box-delivery / area-clearing: pass 1 of the two-pass step (the envs that ran out of pass 0's sim-step budget) and its tail kernels
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;
    hipStream_t st_aux3 = nullptr;  // ... pass 1's kernel with the recurrence test of execute_robot_path, beside the lean one
    hipEvent_t ev_join3 = nullptr;
    int bd_budget = 0;              // sim steps of pass 0 of the two-pass step, 0 = one pass (BP_BD_BUDGET)
    // asynchronous step of box-delivery / area-clearing (bp_bd_step_async / bp_bd_async_drain)
    bool async_open = false;        // a slice is open: envs may be in the middle of an env step (host flag; set by bp_bd_step_async, cleared by the drain and by a reset of all envs)
    int as_epoch = 0;               // serial number of the last asynchronous call (the two launches of a call tell each other's envs apart by it)
    int q_batch = 0;                // > 0: a ready queue with this batch size is open on the slice (bp_bd_queue_*; host flag, as async_open)
    BdQueue q = {};                 // its device arrays, allocated by the first bp_bd_queue_open
    DevParams P;
    DevPtrs D;
    std::vector<void *> allocs;
    size_t lds_bytes = 0, obs_lds_bytes = 0;
    size_t sched_lds = 0;           // dynamic LDS of the scheduler kernels: lds_bytes, or two half-wave images in pairing launches if that is more
    std::string err;
    std::vector<double> goal_raw; // maze: un-normalised wavefront map (info['goal_dt'])
    // box-delivery
    bp_bd_config bdcfg;
    BdParams B;
    BdPtrs Q;
    size_t bd_rmap_lds = 0;
    size_t bd_lds = 0, bd_obs_lds = 0;
    std::vector<bpgeom::BdMaps> bd_maps;
    std::vector<int> bd_map_of_trial;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev; // triples: start, mid, stop
    size_t ev_used = 0;
    unsigned long long *cost_ring = nullptr;   // [BP_COST_RING][2] per-launch (sum, max) of the envs' step cycles while timing is on (k_cost_stats)
    int cost_n = 0;
    // rgb_array frames (bp_set_render_table / bp_render)
    int *r_order = nullptr;           // [T][nbcap] slots bottom first
    unsigned *r_rgb = nullptr;        // [T][nbcap]
    bp_render_prim *r_prims = nullptr;// [BP_RENDER_MAX_PRIMS], layer 0 first
    int r_nunder = 0, r_nover = 0;
    bool r_table = false;
    // state records (bp_state.hpp; bp_save_state / bp_load_state / bp_clone_state)
    unsigned long long scen_hash = 0xCBF29CE484222325ull;   // FNV-1a over the scenario tables as uploaded by the loader
    BpStateLayout st_layout;          // the segment table, built once at load time (state_setup)
    BpStateSeg *st_table = nullptr;   // its device copy
    unsigned long long st_layout_id = 0;
};
#define BP_COST_RING 1024

static int fail(bp_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    return code;
}
#define HIPCHK(h, call)                                                                                       \
    do {                                                                                                      \
        hipError_t _e = (call);                                                                               \
        if (_e != hipSuccess) return fail((h), BP_EHIP, std::string(#call) + ": " + hipGetErrorString(_e));    \
    } while (0)

// Entry points run on the handle's device and leave the calling thread's current device as they found it.
struct DevGuard {
    int prev = -1;
    bool changed = false, ok = true;
    explicit DevGuard(int d)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) { ok = hipSetDevice(d) == hipSuccess; changed = ok; }
    }
    ~DevGuard() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
};
#define BP_DEVICE(h) DevGuard _dg((h)->device); if (!_dg.ok) return fail((h), BP_EHIP, "hipSetDevice failed")

template <typename T>
static int dalloc(bp_handle *h, T **p, size_t n, int fill_byte = 0)
{
    void *q = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(h, BP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    e = hipMemset(q, fill_byte, bytes);
    if (e != hipSuccess) return fail(h, BP_EHIP, std::string("hipMemset: ") + hipGetErrorString(e));
    h->allocs.push_back(q);
    *p = (T *)q;
    return BP_OK;
}

// Host tables to the device.  Every table of a call is allocated (dalloc) before the first is filled: the order in which the loaders have always
// issued these calls, and the traces of profiles/rigid_host pin it.
struct DevTable { const void *src; size_t bytes; void *dev; };
template <typename T>
static DevTable dev_table(const std::vector<T> &v) { return {v.data(), sizeof(T) * v.size(), nullptr}; }
static int upload_tables(bp_handle *h, DevTable *tab, int n)
{
    for (int k = 0; k < n; k++) {
        unsigned char *q;
        if (int rc = dalloc(h, &q, tab[k].bytes)) return rc;
        tab[k].dev = q;
    }
    for (int k = 0; k < n; k++) HIPCHK(h, hipMemcpy(tab[k].dev, tab[k].src, tab[k].bytes, hipMemcpyHostToDevice));
    return BP_OK;
}

static int mvcap_for(int nbcap) { return nbcap > 192 ? nbcap : 192; }
#ifdef BP_PROF
#define BP_PROF_HOST true
#else
#define BP_PROF_HOST false
#endif
static size_t lds_bytes_for(int nbcap, bool box) { return bp_lds_map(nbcap, mvcap_for(nbcap), box, BP_PROF_HOST).total; }

// The chunk boundaries at which a running env may yield (bit k: after k chunks).  A launch without pairing takes no turns during the first 40 % of the step: the
// even finish needs fine turns only towards the end, and every turn costs ~76 us of slot-time -- +1.6 % env-steps/s at 4096 envs, +1.8 % maze, +0.8 %
// at 50 % concentration; pairing launches (-2 % at 5120 envs) keep every boundary.  BP_SCHED_YMASK=<mask> overrides.
static unsigned sched_yield_mask(bool solo_launch, int steps, int chunk)
{
    if (const char *ev = getenv("BP_SCHED_YMASK")) return (unsigned)strtoul(ev, nullptr, 0);
    if (!solo_launch || chunk <= 0) return 0xFFFFFFFFu;
    const int first = (2 * steps + 5 * chunk - 1) / (5 * chunk);   // ceil(0.4 * steps / chunk)
    return first >= 32 ? 0u : (0xFFFFFFFFu << first);
}
// Park images of the scheduler (bp_device.hpp: bp_img_bytes; image_store / image_load in bp_kernels.hpp): one per env, next to sq_carry / sq_moved.  An env that
// yields inside a step is copied out and back verbatim -- LDS block, arbiter registers, sub-step state -- instead of going through the persistent format.
// Bit-identical, and it halves the direct cost of a switch (park 5.4 -> 2.6 us, resume 12.9 -> 7.4 us, no cold first sub-step: profiles/sched_image/), but at ~3 switches
// per env that is ~1 % of the slot-time and the launch followed by less than its run-to-run spread in the same-box A/B: measured-and-not-adopted, OFF by default, BP_SCHED_IMAGE=1 switches it on
// (tools/experiments/README.md).  Pairing launches never use images (a parked env may be continued by a half-wave there).
static int sched_image_setup(bp_handle *h)
{
    const int want = getenv("BP_SCHED_IMAGE") ? atoi(getenv("BP_SCHED_IMAGE")) : 0;
    h->P.sq_image = 0; h->D.sq_img = nullptr;
    if (!want || h->P.pair_mode == 2) return BP_OK;
    h->P.sq_img_lds = (unsigned)h->sched_lds;
    h->P.sq_img_stride = bp_img_bytes(h->P.sq_img_lds);
    unsigned char *d_img;
    int rc = dalloc(h, &d_img, (size_t)h->num_envs * h->P.sq_img_stride);
    if (rc) return rc;
    h->D.sq_img = d_img; h->P.sq_image = 1;
    return BP_OK;
}
// ---- is this process alone on its device? --------------------------------------------------------------------------------------------------------
// A resident kernel holds every wave slot until its launch is over: two PROCESSES that share one GPU can then only alternate by saving and restoring
// 2 048 wavefronts (80 ms per launch measured in a two-rank rehearsal on one device).  One rank per GPU -- the deployment this library is
// built for -- never sees that, but nothing used to detect the other case.  Every handle with resident launches now holds a SHARED advisory lock on a
// per-device file (keyed by the PCI bus id, so that HIP_VISIBLE_DEVICES renumbering does not matter), one descriptor per process and device; "alone" =
// the lock can be converted to EXCLUSIVE without waiting.  Checked at load and every 64 launches (one flock call); while it fails the handle launches the
// dispatcher-driven kernels (bit-identical results, BP_SCHED_PERSIST=0 behaviour) and goes back to resident ones when the other process has left.
// BP_SCHED_PERSIST / BP_PAIR_RESIDENT set explicitly switch the detection off.  Best effort: processes that do not share a /tmp are not seen.
struct ResidentLock { int fd = -1; int refs = 0; };
static std::mutex g_res_mu;
static std::map<std::string, ResidentLock> g_res_locks;

static void resident_acquire(bp_handle *h)
{
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), h->device) != hipSuccess) return;
    for (char *c = bus; *c; c++) if (*c == ':' || *c == '/' || *c == '.') *c = '_';
    const char *dir = getenv("BP_LOCK_DIR");
    const std::string key = std::string(dir ? dir : "/tmp") + "/benchpush_amd.resident." + bus + ".lock";
    std::lock_guard<std::mutex> g(g_res_mu);
    ResidentLock &L = g_res_locks[key];
    if (L.fd < 0) {
        const mode_t um = umask(0);
        L.fd = open(key.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
        umask(um);
        if (L.fd < 0) { g_res_locks.erase(key); return; }   // no lock file: assume the device is ours
        (void)flock(L.fd, LOCK_SH);
    }
    L.refs++;
    h->dev_lock_key = key;
}
static void resident_release(bp_handle *h)
{
    if (h->dev_lock_key.empty()) return;
    std::lock_guard<std::mutex> g(g_res_mu);
    auto it = g_res_locks.find(h->dev_lock_key);
    if (it != g_res_locks.end() && --it->second.refs <= 0) { close(it->second.fd); g_res_locks.erase(it); }
    h->dev_lock_key.clear();
}
// true: some other process holds a share of this device's lock
static bool resident_device_shared(bp_handle *h)
{
    if (h->dev_lock_key.empty()) return false;
    std::lock_guard<std::mutex> g(g_res_mu);
    auto it = g_res_locks.find(h->dev_lock_key);
    if (it == g_res_locks.end()) return false;
    if (flock(it->second.fd, LOCK_EX | LOCK_NB) == 0) { (void)flock(it->second.fd, LOCK_SH); return false; }
    (void)flock(it->second.fd, LOCK_SH);   // a failed conversion may have dropped the shared lock: take it again
    return true;
}
static int device_cus(bp_handle *h)
{
    if (h->num_cus <= 0) {
        hipDeviceProp_t prop;
        HIPCHK(h, hipGetDeviceProperties(&prop, h->device));
        h->num_cus = prop.multiProcessorCount;
    }
    return BP_OK;
}
// Resident wavefronts for a scheduled launch without pairing (k_physics_step_schedl*): one workgroup per wave slot of the device, BP_SCHED_PERSIST=0 goes back to
// one workgroup per task from the hardware dispatcher, BP_SCHED_PERSIST=n > 1 launches n workgroups per slot (the surplus waits for the end and leaves)
static int sched_persist_setup(bp_handle *h)
{
    int rc = device_cus(h);
    if (rc) return rc;
    const int slots = h->num_cus * 4 * (h->P.env_kind == BP_ENV_SHIP_ICE ? BP_SCHED_WAVES : 2);   // 4 SIMDs x 2 wavefronts of 256 VGPRs (x 3 in the occupancy experiment)
    const int pers = getenv("BP_SCHED_PERSIST") ? atoi(getenv("BP_SCHED_PERSIST")) : 1;
    h->sched_persist = pers > 0 ? std::min(h->num_envs, slots * pers) : 0;
    if (h->sched_persist && !h->pd_buf) HIPCHK(h, hipMalloc(&h->pd_buf, sizeof(DevParams) + sizeof(DevPtrs)));
    if (h->sched_persist && !getenv("BP_SCHED_PERSIST")) {
        h->resident_auto = true;
        resident_acquire(h);
        h->device_shared = resident_device_shared(h);
    }
    return BP_OK;
}
extern "C" {

int32_t bp_abi_version(void) { return BP_ABI_VERSION; }
int32_t bp_sizeof_config(void) { return (int32_t)sizeof(bp_config); }

const char *bp_last_error(const bp_handle *h) { return h ? h->err.c_str() : "null handle"; }

int bp_create(const bp_config *cfg, int32_t num_envs, int64_t env_id_offset, int32_t device, bp_handle **out)
{
    if (!cfg || !out || num_envs <= 0) return BP_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BP_ENODEVICE;
    if (!(cfg->damping_pow >= 0.0) || cfg->damping_pow > 1.0) return BP_EINVAL;   // pow(space.damping, dt) of a damping in [0, 1]; != 0 selects the generic kernels (k_physics_*_damp)
    if (cfg->num_ship_verts < 3 || cfg->num_ship_verts > BP_MAX_SHIP_VERTS) return BP_EINVAL;
    if (cfg->steps <= 0 || cfg->iterations <= 0 || cfg->persistence <= 0) return BP_EINVAL;
    if (cfg->env_kind != BP_ENV_SHIP_ICE && cfg->env_kind != BP_ENV_MAZE) return BP_EINVAL;
    if (cfg->env_kind == BP_ENV_MAZE && (cfg->num_wheels < 0 || cfg->num_wheels > BP_MAX_WHEELS)) return BP_EINVAL;
    if (cfg->random_start && cfg->env_kind != BP_ENV_SHIP_ICE) return BP_EINVAL; // per-episode start poses: ship-ice only
    bp_handle *h = new bp_handle();
    h->cfg = *cfg;
    h->num_envs = num_envs;
    h->env_offset = env_id_offset;
    h->device = device;
    h->resettle = (cfg->env_kind == BP_ENV_SHIP_ICE && cfg->random_start != 0); // the settled field depends on the start pose
    DevGuard _dg(device);
    if (!_dg.ok) { delete h; return BP_ENODEVICE; }
    memset(&h->D, 0, sizeof(h->D));
    DevParams &P = h->P;
    memset(&P, 0, sizeof(P));
    P.dt_sub = cfg->dt / cfg->steps;
    P.steps = cfg->steps; P.iterations = cfg->iterations; P.persistence = cfg->persistence; P.settle_steps = cfg->settle_steps;
    if (const char *evp = getenv("BP_DEBUG_PATHS")) P.dbg_paths = atoi(evp); // test hook: force the rarely taken paths of the narrow phase (bp_device.hpp)
    P.bias_lanes = getenv("BP_BIAS_LANES") ? (atoi(getenv("BP_BIAS_LANES")) != 0) : 1;   // 0: sub-steps with a bias term take the bias copy of the solver passes
    P.damping_pow = cfg->damping_pow; P.bias_coef = cfg->bias_coef; P.slop = cfg->slop;
    P.target_speed = cfg->target_speed; P.max_yaw_rate = cfg->max_yaw_rate;
    P.map_w = cfg->map_w; P.map_h = cfg->map_h; P.goal_y = cfg->goal_y; P.m_to_pix = cfg->m_to_pix;
    P.beta = cfg->beta; P.boundary_penalty = cfg->boundary_penalty; P.terminal_reward = cfg->terminal_reward;
    P.local_w = cfg->local_w; P.local_h = cfg->local_h; P.vshift = cfg->vshift; P.obs_range = cfg->obs_range;
    P.skin = 0.06;  // Verlet skin of the neighbour lists (m): a tuning knob only, the lists are an exact broadphase for any value
    P.env_kind = cfg->env_kind;
    P.nkin = (cfg->env_kind == BP_ENV_MAZE) ? 1 + cfg->num_wheels : 1;
    P.goal_x = cfg->goal_x; P.goal_reach = cfg->goal_reach; P.k_increment = cfg->k_increment;
    P.num_envs = num_envs; P.env_offset = env_id_offset;
    P.random_start = (cfg->env_kind == BP_ENV_SHIP_ICE) ? cfg->random_start : 0;
    P.start_x_range = cfg->start_x_range; P.start_seed = cfg->start_seed; P.ship_mass = cfg->ship_mass;
    P.num_ship_verts = cfg->num_ship_verts;
    memcpy(P.ship_verts, cfg->ship_verts, sizeof(P.ship_verts));
    memcpy(P.ship_head, cfg->ship_head, sizeof(P.ship_head));
    memcpy(P.ship_tail, cfg->ship_tail, sizeof(P.ship_tail));
    // OccupancyGrid.__init__ (occupancy_map.py:11-35) with grid cell 1/m_to_pix
    const double grid = 1.0 / cfg->m_to_pix;
    P.grid_w = (int)(cfg->map_w / grid);
    P.grid_h = (int)(cfg->map_h / grid);
    P.obs_h = (int)(cfg->local_h * cfg->m_to_pix);
    P.obs_w = (int)(cfg->local_w * cfg->m_to_pix);
    if ((P.obs_h * P.obs_w) % 4 != 0) { delete h; return BP_EINVAL; }
    if (cfg->env_kind == BP_ENV_MAZE) {
        const int infl = (P.obs_w > P.obs_h ? P.obs_w : P.obs_h) / 2;
        const int nwords = ((P.obs_h + infl) * (P.obs_w + infl) + 31) / 32;
        h->obs_lds_bytes = (size_t)4 * (nwords + ((nwords + 1) & ~1)) + sizeof(double) * 2 * MZ_MAXBOX * 4;
        if (hipFuncSetAttribute((const void *)k_observe_maze, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->obs_lds_bytes) != hipSuccess) { delete h; return BP_EHIP; }
    } else {
        // k_observe composes two window rows as obs_w / 2 whole words per thread group
        if (P.obs_h % 2 != 0 || P.obs_w % 2 != 0 || P.obs_w / 2 > OBS_THREADS_SHIP) { delete h; return BP_EINVAL; }
        h->obs_lds_bytes = (size_t)((P.obs_h * P.obs_w + 15) & ~15) + (size_t)((P.obs_h + 15) & ~15) + sizeof(double) * 2 * OBS_CHUNK * BP_MAXV;
        if (hipFuncSetAttribute((const void *)k_observe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->obs_lds_bytes) != hipSuccess) { delete h; return BP_EHIP; }
    }
    *out = h;
    return BP_OK;
}

int bp_destroy(bp_handle *h)
{
    if (!h) return BP_EINVAL;
    DevGuard _dg(h->device);
    if (h->st_aux) { hipStreamSynchronize(h->st_aux); hipStreamDestroy(h->st_aux); }
    resident_release(h);
    if (h->pd_buf) hipFree(h->pd_buf);
    if (h->st_aux2) { hipStreamSynchronize(h->st_aux2); hipStreamDestroy(h->st_aux2); }
    if (h->st_aux3) { hipStreamSynchronize(h->st_aux3); hipStreamDestroy(h->st_aux3); }
    if (h->ev_join3) hipEventDestroy(h->ev_join3);
    if (h->ev_join2) hipEventDestroy(h->ev_join2);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    for (void *p : h->allocs) hipFree(p);
    for (hipEvent_t e : h->ev) hipEventDestroy(e);
    delete h;
    return BP_OK;
}

// ---- the scenario loader (upload_trials) as a sequence of steps ----------------------------------------------------------------------------------
// Step 1 is host-only: bpgeom::pack_trials (bp_host_scene.hpp), the per-trial bodies as SoA tables with nbcap slots per trial and the scenario hash over them.
// Step 2: the tables to the device (upload_tables)
static_assert(sizeof(bpgeom::P2) == sizeof(d2) && sizeof(bpgeom::D4) == sizeof(double4), "the host tables are uploaded as d2 / double4");
static int upload_trial_tables(bp_handle *h, const bpgeom::TrialTables &tt)
{
    DevTable tab[8] = {dev_table(tt.nb), dev_table(tt.nv), dev_table(tt.kind), dev_table(tt.lv), dev_table(tt.ln), dev_table(tt.mass), dev_table(tt.pose), dev_table(tt.prop)};
    if (int rc = upload_tables(h, tab, 8)) return rc;
    DevPtrs &D = h->D;
    D.sc_nb = (const int *)tab[0].dev; D.sc_nv = (const int *)tab[1].dev; D.sc_kind = (const int *)tab[2].dev;
    D.sc_lv = (const d2 *)tab[3].dev; D.sc_ln = (const d2 *)tab[4].dev;
    D.sc_mass = (const double4 *)tab[5].dev; D.sc_pose = (const double4 *)tab[6].dev; D.sc_prop = (const double4 *)tab[7].dev;
    return BP_OK;
}
// Step 3: per-env state for the E envs plus T settled reset templates (slot E + t = trial t)
static int alloc_env_state(bp_handle *h, int T)
{
    DevPtrs &D = h->D;
    int rc;
    const size_t E = (size_t)h->num_envs + (size_t)T, EB = E * h->nbcap;
    if ((rc = dalloc(h, &D.e_trial, E))) return rc;
    if ((rc = dalloc(h, &D.e_episode, E, 0xFF))) return rc; // -1
    if ((rc = dalloc(h, &D.e_nb, E))) return rc;
    if ((rc = dalloc(h, &D.e_err, E))) return rc;
    if ((rc = dalloc(h, &D.e_flags, E))) return rc;
    if ((rc = dalloc(h, &D.e_prevdist, E))) return rc;
    if ((rc = dalloc(h, &D.e_stamp, E))) return rc;
    if ((rc = dalloc(h, &D.e_currdt, E))) return rc;
    if ((rc = dalloc(h, &D.e_total_work, E))) return rc;
    if ((rc = dalloc(h, &D.e_ke, E))) return rc;
    if ((rc = dalloc(h, &D.e_imp, E))) return rc;
    if ((rc = dalloc(h, &D.e_cnt, E * 4))) return rc;
    if ((rc = dalloc(h, &D.e_cost, E))) return rc;
    if ((rc = dalloc(h, &h->order_buf, E))) return rc;
    D.order = nullptr;
    if ((rc = dalloc(h, &D.pxy, EB))) return rc;
    if ((rc = dalloc(h, &D.ang, EB))) return rc;
    if ((rc = dalloc(h, &D.rot, EB))) return rc;
    if ((rc = dalloc(h, &D.velv, EB))) return rc;
    if ((rc = dalloc(h, &D.velw, EB))) return rc;
    if ((rc = dalloc(h, &D.velb, EB))) return rc;
    if ((rc = dalloc(h, &D.wv, EB * BP_MAXV))) return rc;
    if ((rc = dalloc(h, &D.wn, EB * BP_MAXV))) return rc;
    if ((rc = dalloc(h, &D.pv, EB * BP_MAXV))) return rc;
    if ((rc = dalloc(h, &D.bb, EB))) return rc;
    if ((rc = dalloc(h, &D.fat, EB))) return rc;
    if ((rc = dalloc(h, &D.adj, EB * BP_KADJ))) return rc;
    if ((rc = dalloc(h, &D.adjn, EB))) return rc;
    if ((rc = dalloc(h, &D.hint, EB * BP_KADJ))) return rc;
    if ((rc = dalloc(h, &D.a_key, E * BP_ACAP, 0xFF))) return rc;
    if ((rc = dalloc(h, &D.a_stamp, E * BP_ACAP))) return rc;
    if ((rc = dalloc(h, &D.a_sc, E * BP_ACAP))) return rc;
    if ((rc = dalloc(h, &D.a_h0, E * BP_ACAP))) return rc;
    if ((rc = dalloc(h, &D.a_h1, E * BP_ACAP))) return rc;
    if ((rc = dalloc(h, &D.a_d, E * BP_ACAP * 14))) return rc;
    if ((rc = dalloc(h, &D.e_lastrew, E))) return rc;
    if ((rc = dalloc(h, &D.e_lastflag, E))) return rc;
    if ((rc = dalloc(h, &D.m_acc, E * 8))) return rc;
    if ((rc = dalloc(h, &D.m_rows, E * BP_EPM_COUNT))) return rc;
    if ((rc = dalloc(h, &D.m_ring, E * BP_EPM_RING * BP_EPM_COUNT))) return rc;
    if ((rc = dalloc(h, &D.m_sum, E * BP_EPM_COUNT))) return rc;
    if ((rc = dalloc(h, &D.m_count, E))) return rc;
    if ((rc = dalloc(h, &D.m_open, E))) return rc;
    if ((rc = dalloc(h, &D.clk, (size_t)16))) return rc;
    HIPCHK(h, hipMemset(D.clk, 0, 16 * sizeof(unsigned long long)));
    D.dbg = nullptr; D.dbg_env = -1; D.prof = nullptr;
    return BP_OK;
}
// Step 4, the launch plan.  pair_limits / pair_resident_setup: two environments per wavefront inside the scheduler (pair_mode 2).
static void pair_limits(bp_handle *h)
{
    // two environments per wavefront inside the scheduler: who starts alone, and when a half leaves its pair (pair_should_leave)
    auto envint = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
    h->P.pair_mode = 2;
    // (pace priorities stay on: +0.4 ... +0.9 % in pairing launches)
    // Up to ~6 000 envs per GPU the launch is within a few per cent of the chain of its heaviest env: only envs that are light right now run
    // paired (a medium env beside a mate would become the longest chain), and the eighth of the dispatch order that was heaviest in the previous
    // step starts alone.  From ~7 000 envs the launch is throughput: every env starts in a pair and leaves it at 20 active arbiters or 40 work units per
    // sub-step (same-box sweeps in profiles/r05_pair/ and profiles/r05_sched/pairing_limits_by_batch.txt; on the resident kernel, fresh / steady state:
    // 6144 envs tight 294 k / 306 k against 294 k / 285 k, 7168 envs 300 k / 308 k against 314 k / 310 k, 8192 envs 303 k / 313 k against 323 k / 324 k).
    BpLaunchPolicy &pol = h->pol;
    if (pol.pair_mode != 2)   // (BP_PAIR=2 forced below the default regime)
        bp_policy_pair_limits(pol, 2LL * h->num_envs < (long long)BP_POLICY_LOOSE_FROM_HALF_ROUNDS * pol.wave_slots, h->num_envs);
    h->P.pair_solo = std::min(h->num_envs, std::max(0, envint("BP_PAIR_SOLO", pol.pair_solo)));
    h->P.pp_max_keys = std::min(30, envint("BP_PP_KEYS", 26));
    h->P.pp_max_slots = std::min(PP_NSLOT - 4, envint("BP_PP_SLOTS", 34));
    h->P.pp_max_mv = std::min(PP_MVCAP - 4, envint("BP_PP_MV", 40));
    h->P.pp_max_act = envint("BP_PP_ACT", pol.pp_max_act);
    h->P.pp_max_work = envint("BP_PP_WORK", pol.pp_max_work);
    h->P.pp_rate = envint("BP_PP_RATE", pol.pp_rate);
    h->P.pp_snake = envint("BP_PP_SNAKE", 0);
    h->P.pp_heavy_only = envint("BP_PP_HEAVY_ONLY", 0);
}
// (pairing launches have a resident kernel of their own, k_physics_step_schedr: the kernel that holds both step bodies INLINE lost 4 % at 8192 envs as a
// resident loop -- 266 spilled VGPRs against 203)
static int pair_resident_setup(bp_handle *h)
{
    HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_schedr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->sched_lds));
    const int pr = getenv("BP_PAIR_RESIDENT") ? atoi(getenv("BP_PAIR_RESIDENT")) : 1;   // 0: the dispatcher-driven pair of kernels
    if (pr > 0) {
        h->pair_resident = std::min(h->num_envs, h->pol.wave_slots * pr);
        if (!h->pd_buf) HIPCHK(h, hipMalloc(&h->pd_buf, sizeof(DevParams) + sizeof(DevPtrs)));
        if (!getenv("BP_PAIR_RESIDENT")) { h->resident_auto = true; resident_acquire(h); h->device_shared = resident_device_shared(h); }
    }
    return BP_OK;
}
// Preemptive scheduler (k_physics_step_sched), the default step kernel of a ship-ice handle and of a maze handle with 8-vertex hulls: chunks of 40 sub-steps.
// It pays while the launch is a few rounds of the wave slots (+14 % at 4096 envs; -1 % at 16 384, where the tail is amortised): BP_SCHED=<chunk> forces it,
// BP_SCHED=0 selects the one-wave-per-env kernel.  h->pol and h->pair_mode are settled by the caller.
static int sched_setup(bp_handle *h, bool maze)
{
    int rc;
    // (with paired first tasks the scheduler is what lets an env leave its pair, so it stays on at every batch size: chunks of 100 sub-steps above 8192 envs)
    int ch = h->pol.chunk ? h->pol.chunk : (h->pair_mode == 2 ? 100 : 0);
    if (const char *ev = getenv("BP_SCHED")) ch = atoi(ev);
    if (!(ch > 0 && (h->P.steps + ch - 1) / ch <= SQ_MAXLEV && h->num_envs < (1 << 24))) return BP_OK;
    h->sched_chunk = ch;
    h->P.sq_chunk = ch; h->P.sq_levels = (h->P.steps + ch - 1) / ch;
    if (!maze) {
        // Measured-and-lost scheduler variants (longest-remaining-first keys, hold, static class sets, the launch split over hardware queues: tools/experiments/README.md)
        // are no longer load-time switches (round 6).  Their kernel code paths stay compiled -- taking them out of physics_body / sched_body moved the register allocation
        // of k_physics_step_schedl and cost 1.0 % at 4096 envs, same box, both alternations (tools/experiments/r06_removed_scheduler_variants.diff) -- and are switched off here.
        h->P.sq_hold = 0;
        h->P.sq_lrpt = 0;
        h->P.sq_bw = 9000;
        h->P.sq_hyst = 1;
        h->P.sq_floor = 150;
        h->P.sq_cls = 0;
        h->P.sq_parts = 1;
        h->P.sq_part = 0;
    }
    // pace-based issue priorities (physics_body: pace_prio), per cent of the reference cost for priority 3: +1.5 ... +2.4 % at 4096 envs, flat from 100 to 130
    // (maze, as for ship-ice: +1.6 % at 4096 envs)
    h->P.sq_dynprio = getenv("BP_SCHED_DYNPRIO") ? atoi(getenv("BP_SCHED_DYNPRIO")) : 115;
    h->P.sq_cap = h->num_envs; // an env's home XCD is where its first chunk ran: any share of the envs
    int *d_items, *d_ctr; unsigned *d_carry; unsigned char *d_moved;
    if ((rc = dalloc(h, &d_items, (size_t)SQ_NX * SQ_MAXLEV * h->P.sq_cap))) return rc;
    if ((rc = dalloc(h, &d_ctr, (size_t)SQ_NX * (SQ_MAXLEV + 2) * 2))) return rc;
    if ((rc = dalloc(h, &d_carry, (size_t)h->num_envs * 4))) return rc;
    if ((rc = dalloc(h, &d_moved, (size_t)h->num_envs * h->nbcap))) return rc;
    h->D.sq_items = d_items; h->D.sq_ctr = d_ctr; h->D.sq_carry = d_carry; h->D.sq_moved = d_moved;
    int *d_done, *d_lev, *d_warn, *d_resc;
    if ((rc = dalloc(h, &d_resc, (size_t)1 + SQ_RESCUE))) return rc;
    h->D.sq_rescue = d_resc;
    if ((rc = dalloc(h, &d_done, (size_t)h->num_envs))) return rc;
    if ((rc = dalloc(h, &d_lev, (size_t)h->num_envs))) return rc;
    if ((rc = dalloc(h, &d_warn, (size_t)2))) return rc;
    HIPCHK(h, hipMemset(d_warn, 0, 2 * sizeof(int)));
    h->D.sq_done = d_done; h->D.sq_lev = d_lev; h->D.sq_warn = d_warn;
    unsigned *d_thr;
    if ((rc = dalloc(h, &d_thr, (size_t)1))) return rc;
    HIPCHK(h, hipMemset(d_thr, 0xFF, sizeof(unsigned)));
    h->D.sq_thr = d_thr;
    int *d_sub;
    if ((rc = dalloc(h, &d_sub, (size_t)h->num_envs))) return rc;
    h->D.sq_sub = d_sub;
    if (!maze) {   // (cumulative pairing counters: a maze handle never pairs)
        int *d_pst;
        if ((rc = dalloc(h, &d_pst, (size_t)8))) return rc;
        HIPCHK(h, hipMemset(d_pst, 0, 8 * sizeof(int)));
        h->D.sq_pairstat = d_pst;
    }
#ifdef BP_DEBUG_PATHS   // fault injection lives in the diagnostic twin only: a stray variable in a job environment cannot disturb the product library
    if (const char *ev2 = getenv("BP_SCHED_DEBUG_DROP")) h->P.sq_debug = atoi(ev2);
#endif
    if (h->pair_mode == 2) pair_limits(h);
    // (the per-env kernels k_physics_step / k_physics_reset keep lds_bytes, for which their attribute was set by the loader)
    h->sched_lds = h->pair_mode == 2 ? std::max(h->lds_bytes, (size_t)(2 * PL_HALF)) : h->lds_bytes;
    h->P.sq_ymask = sched_yield_mask(h->P.pair_mode != 2, h->P.steps, h->P.sq_chunk);
    if ((rc = sched_image_setup(h))) return rc;
    if (maze) {
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_sched_maze, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->sched_lds));
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_schedl_maze, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->sched_lds));
    } else {
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_sched, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->sched_lds));
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_schedp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->sched_lds));
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_schedl, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->sched_lds));
    }
    return h->P.pair_mode == 2 ? pair_resident_setup(h) : sched_persist_setup(h);
}
// The plan of a ship-ice handle without damping: pairing mode, then the scheduler.
static int ship_plan(bp_handle *h, const bpgeom::Trials &trials)
{
    const int T = (int)trials.size(), nbcap = h->nbcap;
    bool plain = true; // one kinematic shape (index 0), dynamic shapes without groups otherwise
    for (int t = 0; t < T && plain; t++)
        for (int b = 0; b < (int)trials[t].size(); b++) {
            const int kd = trials[t][b].kind;
            const int bt = (kd >> 16) & 3, grp = (kd >> 8) & 0xFF;
            if (grp != 0 || bt != (b == 0 ? 1 : 0)) { plain = false; break; }
        }
    // two environments per wavefront: the half-wave LDS image is laid out for PP_NBCAP body slots, element offsets are 32-bit
    const bool can_pair = plain && nbcap <= PP_NBCAP &&
                          ((size_t)h->num_envs + (size_t)T) * (size_t)nbcap * BP_MAXV * sizeof(d2) < (size_t)0xFFFFFFFF &&   // 32-bit byte offsets (gA)
                          ((size_t)h->num_envs + (size_t)T) * (size_t)nbcap * BP_KADJ * sizeof(unsigned long long) < (size_t)0xFFFFFFFF;
    // Default: inside the scheduler (mode 2) from 5 120 envs per GPU up, where a launch is throughput (+3.7 % at 5 120, +12 % at 6 144, +19 % at 8 192 and
    // +31 % at 16 384 env-steps/s over the resident solo scheduler, same box).  Below, the launch follows the chains of its heaviest envs and the scheduler's rotation, not the sum of the work: pairing
    // the light envs saves a tenth of the wave-instructions and moves the launch by 0 ... +2.5 % at 4 096 envs (profiles/r05_pair/), -2 % at 2 048 --
    // and the kernel that holds both step bodies runs the solo body 6 % slower -- so those handles keep the lean one-env-per-wavefront scheduler kernel.
    // BP_PAIR=0 / 1 / 2 overrides.
    if (int rc = device_cus(h)) return rc;
    // regime boundaries in rounds of the device's wave slots, not in envs (bp_policy.hpp): pairing from 2.5 rounds, loose limits from 3.5, no scheduler
    // without pairing above 4 -- 5 120 / 7 168 / 8 192 envs on the 256 CUs they were measured on
    h->pol = bp_launch_policy(h->num_envs, h->num_cus, can_pair, false);
    h->pair_mode = h->pol.pair_mode;
    if (const char *evp = getenv("BP_PAIR")) h->pair_mode = can_pair ? atoi(evp) : 0;
    if (h->pair_mode == 1) {
        h->P.pair_mode = 1;
        if (const char *evs = getenv("BP_PAIR_SNAKE")) h->P.pair_solo = atoi(evs);
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_pair, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * PL_HALF)));
    }
    if (plain) { if (int rc = sched_setup(h, false)) return rc; }
    if (h->pair_mode == 2 && h->P.pair_mode != 2) h->pair_mode = 0;   // pairing inside the scheduler needs the scheduler
    return BP_OK;
}
// The kernel of each role, chosen once (bp_handle::k).  maze8: a maze whose hulls all have <= 8 vertices, kernels instantiated with 8-vertex loops
static RigidKernels rigid_kernels(const bp_handle *h, bool maze8)
{
    RigidKernels k;
    if (h->damp) { k.step = k_physics_step_damp; k.reset = k_physics_reset_damp; }   // (no scheduler)
    else if (maze8) { k.step = k_physics_step_maze; k.sched = k_physics_step_sched_maze; k.resident = k_physics_step_schedl_maze; k.reset = k_physics_reset_maze; }
    else { k.step = k_physics_step; k.sched = k_physics_step_sched; k.resident = h->P.pair_mode == 2 ? k_physics_step_schedr : k_physics_step_schedl; k.reset = k_physics_reset; }
    return k;
}
// Step 5: settle every trial once into its reset template (new space + bodies + 1000 sub-steps, ship_ice_env.py:109-220); reset() copies from these
static int settle_templates(bp_handle *h)
{
    hipLaunchKernelGGL(h->k.reset, dim3(h->num_trials), dim3(64), h->lds_bytes, 0, h->P, h->D, (const unsigned char *)nullptr, (double *)nullptr, 1);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipDeviceSynchronize());
    h->loaded = true;
    return BP_OK;
}
// Common tail of the scenario loaders: SoA upload of the per-trial bodies, per-env state allocation, the launch plan, and one settle of
// every trial into its reset template (state slot num_envs + t).  bp_bd_load passes settle = false: it plans and settles on its own.
static int upload_trials(bp_handle *h, const bpgeom::Trials &trials, bool settle = true)
{
    const int T = (int)trials.size();
    const int nbcap = bpgeom::trials_nbcap(trials);
    if (nbcap > 60000) return fail(h, BP_EINVAL, "too many bodies");
    h->nbcap = nbcap;
    h->num_trials = T;
    h->P.nbcap = nbcap;
    h->P.mvcap = mvcap_for(nbcap);
    h->P.num_trials = T;
    h->lds_bytes = lds_bytes_for(nbcap, h->P.env_kind == BP_ENV_BOX);
    if (h->lds_bytes > 160 * 1024) return fail(h, BP_EINVAL, "nb_cap too large for LDS");
    // the candidate cache (LdsCtx::cc, bp_physics.hpp step 3) packs both body indices of a pair into BP_CC_IDX_BITS bits each
    if (nbcap >= (1 << BP_CC_IDX_BITS)) return fail(h, BP_EINVAL, "nb_cap exceeds the candidate cache's body-index field (16384 bodies per env)");
    int rc;
    bpgeom::TrialTables tt;
    if (const char *e = bpgeom::pack_trials(trials, nbcap, tt, h->scen_hash)) return fail(h, BP_EINVAL, e);
    if ((rc = upload_trial_tables(h, tt))) return rc;
    if ((rc = alloc_env_state(h, T))) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
    HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_reset, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
    h->damp = h->P.damping_pow != 0.0;
    if (h->damp) {
        // space.damping != 0: one generic pair of kernels for ship-ice and maze handles; settle every trial once with it
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_damp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_reset_damp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
    } else if (h->P.env_kind == BP_ENV_SHIP_ICE && h->P.nkin == 1 && nbcap < 16384) {
        if ((rc = ship_plan(h, trials))) return rc;
    }
    if (!settle) return BP_OK;
    bool maze8 = !h->damp && h->P.env_kind == BP_ENV_MAZE;
    for (int v : tt.nv) if (v > 8) maze8 = false;
    if (maze8) {
        if ((rc = device_cus(h))) return rc;
        h->pol = bp_launch_policy(h->num_envs, h->num_cus, false, true);
        if ((rc = sched_setup(h, true))) return rc;   // preemptive scheduler, as for ship-ice
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_step_maze, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
        HIPCHK(h, hipFuncSetAttribute((const void *)k_physics_reset_maze, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
    }
    h->k = rigid_kernels(h, maze8);
    return settle_templates(h);
}

// State records: the segment table over this handle's arrays, its device copy and the layout id (bp_state.hpp).  Called once, at the end of every loader.
static int state_setup(bp_handle *h)
{
    const bool box = h->P.env_kind == BP_ENV_BOX;
    const int cells = box ? h->B.SH * h->B.SW : 0;
    h->st_layout = bp_state_layout(h->D, h->Q, h->nbcap, box, cells);
    const BpStateLayout &L = h->st_layout;
    if (L.nseg >= BP_STATE_MAXSEG || (L.bytes >> 4) >= 0xFFFFFFFFull) return fail(h, BP_EINVAL, "state record layout out of range");
    unsigned long long id = bp_state_structure_id(L, h->P.env_kind, box ? h->bdcfg.task : 0, h->nbcap, cells);
    if (box) id = bp_fnv1a(&h->bdcfg, sizeof(h->bdcfg), id);
    else id = bp_fnv1a(&h->cfg, sizeof(h->cfg), id);
    h->st_layout_id = bp_fnv1a_i64((long long)h->scen_hash, id);
    int rc = dalloc(h, &h->st_table, (size_t)BP_STATE_MAXSEG);
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(h->st_table, L.seg, sizeof(BpStateSeg) * L.nseg, hipMemcpyHostToDevice));
    return BP_OK;
}

// The loaders: argument and state checks, the host-only scene builder (bp_host_scene.hpp), then the device steps.
int bp_load_scenarios(bp_handle *h, int32_t T, int32_t F, int32_t V, const double *verts, const int32_t *counts,
                      const double *centres, const double *starts, const int32_t *nfloes)
{
    if (!h || T <= 0 || F < 0 || V <= 0 || !starts || !nfloes) return BP_EINVAL;
    if (h->loaded) return fail(h, BP_ESTATE, "scenarios already loaded");
    if (h->P.env_kind != BP_ENV_SHIP_ICE) return fail(h, BP_ESTATE, "handle was created for another environment");
    BP_DEVICE(h);
    bpgeom::Trials trials;
    if (const char *e = bpgeom::ship_ice_scene(h->cfg, T, F, V, verts, counts, centres, starts, nfloes, trials)) return fail(h, BP_EINVAL, e);
    const int rc_up = upload_trials(h, trials);
    return rc_up ? rc_up : state_setup(h);
}

int bp_load_maze(bp_handle *h, int32_t T, int32_t nbox, const double *centres, int32_t nwalls, const double *walls, const double *start)
{
    if (!h || T <= 0 || nbox < 0 || nwalls < 0 || nwalls > 16 || !walls || !start || (nbox > 0 && !centres)) return BP_EINVAL;
    if (h->loaded) return fail(h, BP_ESTATE, "scenarios already loaded");
    if (h->P.env_kind != BP_ENV_MAZE) return fail(h, BP_ESTATE, "handle was created for another environment");
    BP_DEVICE(h);
    bpgeom::MazeScene sc;
    if (const char *e = bpgeom::maze_scene(h->cfg, h->P.grid_h, h->P.grid_w, T, nbox, centres, nwalls, walls, start, sc)) return fail(h, BP_EINVAL, e);
    int rc;
    DevTable maps[2] = {dev_table(sc.norm), dev_table(sc.wall)};
    if ((rc = upload_tables(h, maps, 2))) return rc;
    h->D.dist_map = (const double *)maps[0].dev; h->D.wall_map = (const unsigned char *)maps[1].dev;
    DevTable pk = dev_table(sc.obs_map);
    if ((rc = upload_tables(h, &pk, 1))) return rc;
    h->D.maze_obs_map = (const double *)pk.dev;
    DevTable raw = dev_table(sc.raw);
    if ((rc = upload_tables(h, &raw, 1))) return rc;
    h->D.goal_raw = (const double *)raw.dev;
    h->goal_raw = sc.raw;
    h->scen_hash = bpgeom::maze_scene_hash(sc, h->scen_hash);
    const int rc_up = upload_trials(h, sc.trials);
    return rc_up ? rc_up : state_setup(h);
}

int bp_get_goal_map(bp_handle *h, double *out_host, int32_t *grid_h, int32_t *grid_w)
{
    if (!h) return BP_EINVAL;
    if (h->goal_raw.empty()) return fail(h, BP_ESTATE, "no goal map (not a maze handle or not loaded)");
    if (out_host) memcpy(out_host, h->goal_raw.data(), sizeof(double) * h->goal_raw.size());
    if (grid_h) *grid_h = h->P.grid_h;
    if (grid_w) *grid_w = h->P.grid_w;
    return BP_OK;
}

// python's round(x, 2) (ship_ice_env.py:337-339 rounds info['state']): the double nearest to x rounded to two decimals, ties of the
// exact value to even.  x * 100 is taken exactly (product + fma residual), so a product that only *rounds* onto a tie is not one.
__device__ __forceinline__ double bp_round2(double x)
{
    const double y = x * 100.0;
    const double e = __builtin_fma(x, 100.0, -y);
    double k = __builtin_rint(y);
    if (__builtin_fabs(y - k) == 0.5 && e != 0.0) { const double lo = __builtin_floor(y); k = (e > 0.0) ? lo + 1.0 : lo; }
    return k / 100.0;
}
__global__ __launch_bounds__(256) void k_debug_round2(const double *__restrict__ in, double *__restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = bp_round2(in[i]);
}

// ShipIceMetric.reset / update (ship_ice_metric.py:26-69; shared arithmetic in benchpush_amd/metrics/interactive_nav.py) for every env,
// one thread per env, after the physics kernel of bp_step (mode 0) or the reset kernel of bp_reset (mode 1).
__device__ __forceinline__ void episode_metrics_env(const DevParams &P, const DevPtrs &D, const int mode, const unsigned char *__restrict__ mask, const int env)
{
    if (env >= P.num_envs) return;
    double *a = D.m_acc + (size_t)env * 8;
    const d2 p = D.pxy[(size_t)env * P.nbcap];
    const double x = bp_round2(p.x), y = bp_round2(p.y);
    auto emit = [&](double success) {
        const double l0 = a[1], L = a[4], work = a[6];
        const double own = P.ship_mass * l0;
        double *r = D.m_rows + (size_t)env * BP_EPM_COUNT;
        r[BP_EPM_EFFICIENCY] = (success != 0.0) ? L / l0 : 0.0;   // compute_efficiency_score
        r[BP_EPM_EFFORT] = own / (own + work);                    // compute_effort_score
        r[BP_EPM_REWARD] = a[0]; r[BP_EPM_SUCCESS] = success; r[BP_EPM_LENGTH] = a[5]; r[BP_EPM_TOTAL_WORK] = work;
        // the lists of BaseMetric (base_metric.py:12-16): ring of the last episodes and running sums over all of them
        const unsigned n = D.m_count[env];
        double *ring = D.m_ring + ((size_t)env * BP_EPM_RING + n % BP_EPM_RING) * BP_EPM_COUNT, *sum = D.m_sum + (size_t)env * BP_EPM_COUNT;
        for (int q = 0; q < BP_EPM_COUNT; q++) { ring[q] = r[q]; sum[q] += r[q]; }
        D.m_count[env] = n + 1u;
    };
    if (mode == 1) {
        if (mask != nullptr && mask[env] == 0) return;
        if (D.m_open[env] && a[5] > 0.0) emit(0.0);   // reset of a running episode: eps_complete by truncation
        double L = P.goal_y - y;                      // ShipIceMetric: goal line - start y (ship_ice_metric.py:52)
        if (P.env_kind == BP_ENV_MAZE) {              // MazeNamoMetric: wavefront length at the start pixel (maze_namo_metric.py:68-75)
            const int px = (int)(x * P.m_to_pix), py = (int)(y * P.m_to_pix);
            L = (px >= 0 && px < P.grid_w && py >= 0 && py < P.grid_h) ? D.goal_raw[(size_t)py * P.grid_w + px] / P.m_to_pix : 0.0;
        }
        a[0] = 0.0; a[1] = 0.0; a[2] = x; a[3] = y; a[4] = L; a[5] = 0.0; a[6] = 0.0; a[7] = 0.0;
        D.m_open[env] = 1;
        return;
    }
    if (!D.m_open[env]) return; // stepped past its end without a reset: nothing to account
    const int fl = D.e_lastflag[env];
    const double dx = a[2] - x, dy = a[3] - y;
    a[0] += D.e_lastrew[env];
    a[1] += __builtin_sqrt(dx * dx + dy * dy);
    a[2] = x; a[3] = y;
    a[5] += 1.0;
    a[6] = D.e_total_work[env];
    a[7] = (double)((fl >> 1) & 1);
    if (fl & 1) { emit(a[7]); D.m_open[env] = 0; }
}
__global__ __launch_bounds__(256) void k_episode_metrics(const DevParams P, const DevPtrs D, const int mode, const unsigned char *__restrict__ mask)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    // bp_get_clock_stamps: the thread of env 0 times its own stay in this kernel with both counters and adds the two differences to running sums.  Counter
    // values of different launches must not be subtracted from each other: the shader-clock counters that two launches read are not synchronised (their
    // offsets, ~1e8 cycles, turned a span of 20 ms into clocks between -3 and 8 GHz), whereas both ends of one wave's stay are read in one place.
    unsigned long long c0 = 0ull, r0 = 0ull;
    if (env == 0) { c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    episode_metrics_env(P, D, mode, mask, env);
    if (env == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the stay includes the round trips of the env's own loads and stores
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        D.clk[0] += c1 - c0; D.clk[1] += r1 - r0;
    }
}

#include "bp_taskmetric.hpp"   // k_task_metrics: the same for box-delivery / area-clearing handles (needs bp_round2)

enum { MODE_ASYNC = 2, MODE_DRAIN = 3 };   // box-delivery / area-clearing: bp_bd_step_async, bp_bd_async_drain
struct StepOut { unsigned char *obs; double *reward; unsigned char *term, *trunc; double *info; };   // the output rows of a launch, null where a call has none
struct AsyncArgs {                         // what those two calls hand to launch() beside the step's outputs
    int budget;                            // sim steps per env and call (0: no limit, the drain)
    unsigned char *ready;                  // [E]
    int *slices;                           // [E]
};
// The side streams and events of a box-delivery / area-clearing step, created when first needed: the robot map beside the finish kernel (st_aux, ev_fork,
// ev_join); two_pass: also those of the second pass of the two-pass step.
static int bd_side_streams(bp_handle *h, bool two_pass)
{
    if (!h->st_aux) HIPCHK(h, hipStreamCreateWithFlags(&h->st_aux, hipStreamNonBlocking));
    if (!h->ev_fork) HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    if (!h->ev_join) HIPCHK(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    if (!two_pass) return BP_OK;
    if (!h->st_aux2) HIPCHK(h, hipStreamCreateWithFlags(&h->st_aux2, hipStreamNonBlocking));
    if (!h->ev_join2) HIPCHK(h, hipEventCreateWithFlags(&h->ev_join2, hipEventDisableTiming));
    if (!h->st_aux3) HIPCHK(h, hipStreamCreateWithFlags(&h->st_aux3, hipStreamNonBlocking));
    if (!h->ev_join3) HIPCHK(h, hipEventCreateWithFlags(&h->ev_join3, hipEventDisableTiming));
    return BP_OK;
}
// The task's finish kernel for the envs that Bx selects; init: the episode-start bookkeeping of the trials' template slots instead (bp_bd_load).
static int bd_finish(bp_handle *h, const BdParams &Bx, hipStream_t s, const StepOut &out, int init = 0)
{
    const dim3 grid(init ? h->num_trials : h->num_envs);
    if (h->B.task == 1) hipLaunchKernelGGL(k_ac_finish, grid, dim3(64), h->bd_lds, s, h->P, h->D, Bx, h->Q, init, init, out.reward, out.term, out.trunc, out.info);
    else hipLaunchKernelGGL(k_bd_finish, grid, dim3(64), h->bd_lds, s, h->P, h->D, Bx, h->Q, init, init, out.reward, out.term, out.trunc, out.info);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
static int bd_observe(bp_handle *h, const BdParams &Bx, hipStream_t s, const unsigned char *mask, unsigned char *obs)
{
    hipLaunchKernelGGL(k_bd_observe, dim3(h->num_envs), dim3(BDO_THREADS), h->bd_obs_lds, s, h->P, h->D, Bx, h->Q, mask, obs);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
// The tail of an env step for the envs that Bx selects (Q.unfin[e] == Bx.sel_want; -1: all): the robot's spfa map, which needs only the robot pose, on `side`
// beside the finish kernel on `st`, the join, and with `obs` their observation.  The caller has recorded ev_fork behind the physics kernel.  side == st: the
// stream orders the two by itself, the map first, and one error check serves both launches.
static int bd_tail(bp_handle *h, const BdParams &Bx, hipStream_t st, hipStream_t side, const StepOut &out, unsigned char *obs)
{
    if (side != st) HIPCHK(h, hipStreamWaitEvent(side, h->ev_fork, 0));
    hipLaunchKernelGGL(k_bd_robot_map, dim3(h->num_envs), dim3(BDR_THREADS), h->bd_rmap_lds, side, h->P, h->D, Bx, h->Q, 0);
    if (side != st) {
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(h->ev_join, side));
    }
    if (int rc = bd_finish(h, Bx, st, out)) return rc;
    if (side != st) HIPCHK(h, hipStreamWaitEvent(st, h->ev_join, 0));
    return obs ? bd_observe(h, Bx, st, nullptr, obs) : BP_OK;
}
static int bd_physics(bp_handle *h, const BdParams &Bx, hipStream_t s)
{
    if (h->damp) hipLaunchKernelGGL(k_bd_physics_damp, dim3(h->num_envs), dim3(64), h->lds_bytes, s, h->P, h->D, Bx, h->Q);
    else hipLaunchKernelGGL(k_bd_physics, dim3(h->num_envs), dim3(64), h->lds_bytes, s, h->P, h->D, Bx, h->Q);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
// Two-pass step: a launch of k_bd_physics lasts as long as its slowest env, and the slowest are single wavefronts inside the reference's own 10 001-step loops
// (DESIGN.md 4c).  Pass 0 gives every env `bd_budget` sim steps; the envs that are done -- all but a handful -- go through the tail on the caller's stream while
// pass 1 carries the others to their end on a third stream, followed by the same kernels for that group.  Results are those of the single pass (the loop state
// travels through Q.rs_*, bodies and arbiters through the ordinary store / load of a step boundary).  Returns with both groups joined on `st`.
static int bd_step_two_pass(bp_handle *h, hipStream_t st, const StepOut &out, unsigned char *obs)
{
    const int E = h->num_envs;
    BdParams B0 = h->B, B1 = h->B, Bs0 = h->B, Bs1 = h->B;
    B0.budget = h->bd_budget; B0.pass = 0; B1.pass = 1; Bs0.sel_want = 0; Bs1.sel_want = 1;
    if (int rc = bd_physics(h, B0, st)) return rc;
    HIPCHK(h, hipEventRecord(h->ev_fork, st));
    // group 1 (unfinished): third stream, its tail on that stream alone
    HIPCHK(h, hipStreamWaitEvent(h->st_aux2, h->ev_fork, 0));
    if (!h->damp && h->B.cycle_skip > 0) {
        // the envs that stopped inside execute_robot_path: the kernel with the recurrence test (a robot pushing against a wall is over after a
        // handful of sim steps there); then the others -- the reference's own until-still loops -- on the lean kernel
        // (side by side on two streams: an env that pushes boxes through a long path is neither)
        BdParams B1p = B1, B1s = B1;
        B1p.resume_sel = 1; B1s.resume_sel = 2;
        HIPCHK(h, hipStreamWaitEvent(h->st_aux3, h->ev_fork, 0));
        hipLaunchKernelGGL(k_bd_physics_resume, dim3(E), dim3(64), h->lds_bytes, h->st_aux3, h->P, h->D, B1p, h->Q);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(h->ev_join3, h->st_aux3));
        hipLaunchKernelGGL(k_bd_physics, dim3(E), dim3(64), h->lds_bytes, h->st_aux2, h->P, h->D, B1s, h->Q);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamWaitEvent(h->st_aux2, h->ev_join3, 0));
        HIPCHK(h, hipGetLastError());   // (the check that ends either arm, as bd_physics does in the other)
    } else if (int rc = bd_physics(h, B1, h->st_aux2)) return rc;
    if (int rc = bd_tail(h, Bs1, h->st_aux2, h->st_aux2, out, obs)) return rc;
    HIPCHK(h, hipEventRecord(h->ev_join2, h->st_aux2));
    // group 0 (done in pass 0): the caller's stream, the robot map beside the finish kernel as in the one-pass step
    if (int rc = bd_tail(h, Bs0, st, h->st_aux, out, obs)) return rc;
    HIPCHK(h, hipStreamWaitEvent(st, h->ev_join2, 0));
    return BP_OK;
}
// Asynchronous step (bp_bd_step_async / bp_bd_async_drain, DESIGN.md "Asynchronous step"): idle envs are planned and started, busy ones resumed, each runs at
// most `as.budget` sim steps; the envs whose env step ended (group byte 0) go through the tail exactly as in the one-pass step.
// (Dispatch order: h->D.order is what the last lock-step step left, or none -- any permutation serves.)
static int bd_step_slice(bp_handle *h, int mode, const double *actions, hipStream_t st, const StepOut &out, unsigned char *obs, const AsyncArgs &as)
{
    const int E = h->num_envs;
    if (int rc = bd_side_streams(h, false)) return rc;
    const int epoch = ++h->as_epoch;
    BdParams Bp = h->B, Bl = h->B, Bt = h->B;
    Bp.pass = Bl.pass = (mode == MODE_ASYNC) ? 2 : 3;
    Bp.budget = Bl.budget = (mode == MODE_ASYNC) ? as.budget : 0;
    Bp.resume_sel = 1; Bl.resume_sel = 2; Bt.sel_want = 0;
    if (mode == MODE_ASYNC) {
        hipLaunchKernelGGL(k_bd_plan_async, dim3(E), dim3(64), h->bd_lds, st, h->P, h->D, h->B, h->Q, actions);
        HIPCHK(h, hipGetLastError());
    }
    // first the busy envs that stopped inside execute_robot_path (the kernel with the recurrence test), then every other env on the lean kernel
    if (h->B.cycle_skip > 0) {
        hipLaunchKernelGGL(k_bd_slice_resume, dim3(E), dim3(64), h->lds_bytes, st, h->P, h->D, Bp, h->Q, as.ready, as.slices, epoch);
        HIPCHK(h, hipGetLastError());
    } else Bl.resume_sel = 0;
    hipLaunchKernelGGL(k_bd_slice, dim3(E), dim3(64), h->lds_bytes, st, h->P, h->D, Bl, h->Q, as.ready, as.slices, epoch);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev_fork, st));
    if (int rc = bd_tail(h, Bt, st, h->st_aux, out, nullptr)) return rc;
    // episode metrics: only the envs that emitted a transition in this call are accounted
    hipLaunchKernelGGL(k_task_metrics, dim3((E + 255) / 256), dim3(256), 0, st, h->P, h->B, h->D, h->Q, 0, (const unsigned char *)nullptr, (const unsigned char *)as.ready);
    HIPCHK(h, hipGetLastError());
    return obs ? bd_observe(h, Bt, st, nullptr, obs) : BP_OK;   // only the envs that emitted a transition get a new observation
}
// A launch on a box-delivery / area-clearing handle.  e1, e2: the timing events of launch(), null without timing.
static int launch_box(bp_handle *h, int mode, const double *actions, const unsigned char *mask, const StepOut &out, hipStream_t st, bool physics, bool raster,
                      const AsyncArgs *as, hipEvent_t e1, hipEvent_t e2)
{
    const int E = h->num_envs;
    unsigned char *obs = raster ? out.obs : nullptr;   // the observation still to enqueue
    if (physics && mode == MODE_STEP) {
        if (h->steps_done) {
            hipLaunchKernelGGL(k_make_order, dim3(1), dim3(1024), 0, st, (const unsigned *)h->D.e_cost, h->order_buf, E, (unsigned *)nullptr);
            HIPCHK(h, hipGetLastError());
            h->D.order = h->order_buf;
        }
        h->steps_done = true;
        hipLaunchKernelGGL(k_bd_plan, dim3(E), dim3(64), h->bd_lds, st, h->P, h->D, h->B, h->Q, actions);
        HIPCHK(h, hipGetLastError());
        if (int rc = bd_side_streams(h, true)) return rc;
        if (h->bd_budget > 0) {
            if (int rc = bd_step_two_pass(h, st, out, obs)) return rc;
            obs = nullptr;   // both groups' observations are on their way
        } else {
            if (int rc = bd_physics(h, h->B, st)) return rc;
            HIPCHK(h, hipEventRecord(h->ev_fork, st));
            if (int rc = bd_tail(h, h->B, st, h->st_aux, out, nullptr)) return rc;
        }
        // episode metrics of the step (TaskDrivenMetric): both groups' finish kernels have joined the caller's stream
        hipLaunchKernelGGL(k_task_metrics, dim3((E + 255) / 256), dim3(256), 0, st, h->P, h->B, h->D, h->Q, 0, (const unsigned char *)nullptr, (const unsigned char *)nullptr);
        HIPCHK(h, hipGetLastError());
    } else if (physics && (mode == MODE_ASYNC || mode == MODE_DRAIN)) {
        if (int rc = bd_step_slice(h, mode, actions, st, out, obs, *as)) return rc;
        obs = nullptr;
    } else if (physics) {
        hipLaunchKernelGGL(k_reset_copy, dim3(E), dim3(256), 0, st, h->P, h->D, mask, (double *)nullptr);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(k_bd_reset_copy, dim3(E), dim3(256), 0, st, h->P, h->D, h->B, h->Q, mask, out.info);
        HIPCHK(h, hipGetLastError());
        // closes the running episodes of the mask and takes the new episode's snapshot (start position, box areas / centroids) from the reset state
        hipLaunchKernelGGL(k_task_metrics, dim3((E + 255) / 256), dim3(256), 0, st, h->P, h->B, h->D, h->Q, 1, mask, (const unsigned char *)nullptr);
        HIPCHK(h, hipGetLastError());
    }
    // (existing behaviour: in the two-pass and the asynchronous mode the observation is enqueued before e1, so the timers count it as physics)
    if (e1) HIPCHK(h, hipEventRecord(e1, st));
    if (obs) { if (int rc = bd_observe(h, h->B, st, mask, obs)) return rc; }
    if (e2) HIPCHK(h, hipEventRecord(e2, st));
    return BP_OK;
}
// A launch on a ship-ice / maze handle.
static int launch_rigid(bp_handle *h, int mode, const double *actions, const unsigned char *mask, const StepOut &out, hipStream_t st, bool physics, bool raster,
                        hipEvent_t e1, hipEvent_t e2)
{
    unsigned char *obs = out.obs, *term = out.term, *trunc = out.trunc;
    double *reward = out.reward, *info = out.info;
    if (physics) {
        if (mode == MODE_STEP && h->steps_done) { // heaviest-first dispatch order from the previous step's per-env cycles
            hipLaunchKernelGGL(k_make_order, dim3(1), dim3(1024), 0, st, (const unsigned *)h->D.e_cost, h->order_buf, h->num_envs, h->D.sq_thr);
            HIPCHK(h, hipGetLastError());
            h->D.order = h->order_buf;
        }
        if (mode == MODE_STEP) h->steps_done = true;
        if (mode == MODE_STEP && h->pair_mode == 1 && h->D.dbg == nullptr)
            hipLaunchKernelGGL(k_physics_step_pair, dim3((h->num_envs + 1) / 2), dim3(64), 2 * PL_HALF, st, h->P, h->D, actions, reward, term, trunc, info);
        else if (mode == MODE_STEP && h->sched_chunk > 0 && h->D.dbg == nullptr) {
            // preemptive scheduler: one workgroup per (env, chunk) task (most leave at once: only parked envs need a second workgroup)
            hipLaunchKernelGGL(k_sched_init, dim3(16), dim3(1024), 0, st, h->P, h->D);
            HIPCHK(h, hipGetLastError());
            // resident launches only while this process has the device to itself (see resident_device_shared)
            if (h->resident_auto && (++h->launches & 63u) == 0) h->device_shared = resident_device_shared(h);
            const bool resident_ok = !(h->resident_auto && h->device_shared);
            // resident wavefronts: one workgroup per wave slot for the whole launch (sched_persist_setup); of a pairing launch: one kernel, the two step bodies as
            // functions of their own (pair_resident_setup)
            const int resident = !resident_ok ? 0 : h->P.pair_mode == 2 ? h->pair_resident : h->sched_persist;
            if (resident > 0) {
                // the launch constants go through device memory (see sched_resident)
                DevParams *Pg = (DevParams *)h->pd_buf;
                DevPtrs *Dg = (DevPtrs *)((char *)h->pd_buf + sizeof(DevParams));
                hipLaunchKernelGGL(k_store_params, dim3(1), dim3(64), 0, st, h->P, h->D, Pg, Dg);
                HIPCHK(h, hipGetLastError());
                hipLaunchKernelGGL(h->k.resident, dim3(resident), dim3(64), h->sched_lds, st, Pg, Dg, actions, reward, term, trunc, info);
            } else if (h->P.pair_mode == 2) {
                // (BP_PAIR_RESIDENT=0) a pairing launch as two kernels side by side: the envs that start alone on the lean solo code (second stream), everything else -- paired
                // first tasks, the workgroups that serve the queues -- in the kernel that holds both step bodies
                if (!h->st_aux) {
                    HIPCHK(h, hipStreamCreateWithFlags(&h->st_aux, hipStreamNonBlocking));
                    HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
                    HIPCHK(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
                }
                if (h->P.pair_solo > 0) {
                    HIPCHK(h, hipEventRecord(h->ev_fork, st));
                    HIPCHK(h, hipStreamWaitEvent(h->st_aux, h->ev_fork, 0));
                    hipLaunchKernelGGL(k_physics_step_sched, dim3(h->P.pair_solo), dim3(64), h->sched_lds, h->st_aux, h->P, h->D, actions, reward, term, trunc, info);
                    HIPCHK(h, hipGetLastError());
                    HIPCHK(h, hipEventRecord(h->ev_join, h->st_aux));
                }
                hipLaunchKernelGGL(k_physics_step_schedp, dim3(h->num_envs * h->P.sq_levels), dim3(64), h->sched_lds, st, h->P, h->D, actions, reward, term, trunc, info);
                HIPCHK(h, hipGetLastError());
                if (h->P.pair_solo > 0) HIPCHK(h, hipStreamWaitEvent(st, h->ev_join, 0));
            } else
                hipLaunchKernelGGL(h->k.sched, dim3(h->num_envs * h->P.sq_levels), dim3(64), h->sched_lds, st, h->P, h->D, actions, reward, term, trunc, info);
            HIPCHK(h, hipGetLastError());
            // completion launch: workgroup b finishes the b-th env that the scheduled launch left unfinished (scheduler watchdog); normally all leave at once
#ifdef BP_DEBUG_PATHS
            static const bool completion = !(getenv("BP_SCHED_COMPLETION") && atoi(getenv("BP_SCHED_COMPLETION")) == 0);   // diagnostic switch (twin library only)
#else
            constexpr bool completion = true;
#endif
            if (completion) {
                hipLaunchKernelGGL(k_sched_scan, dim3(1), dim3(256), 0, st, h->P, h->D);
                HIPCHK(h, hipGetLastError());
                DevParams PC = h->P;
                PC.sq_mode = 1;
                hipLaunchKernelGGL(h->k.sched, dim3(std::min(h->num_envs, SQ_RESCUE)), dim3(64), h->sched_lds, st, PC, h->D, actions, reward, term, trunc, info);
            }
        }
        else if (mode == MODE_STEP)
            hipLaunchKernelGGL(h->k.step, dim3(h->num_envs), dim3(64), h->lds_bytes, st, h->P, h->D, actions, reward, term, trunc, info);
        else if (h->resettle)
            hipLaunchKernelGGL(h->k.reset, dim3(h->num_envs), dim3(64), h->lds_bytes, st, h->P, h->D, mask, info, 0);
        else
            hipLaunchKernelGGL(k_reset_copy, dim3(h->num_envs), dim3(256), 0, st, h->P, h->D, mask, info);
        HIPCHK(h, hipGetLastError());
        if (mode == MODE_STEP && h->timing && h->cost_ring && h->cost_n < BP_COST_RING) {
            hipLaunchKernelGGL(k_cost_stats, dim3(1), dim3(1024), 0, st, (const unsigned *)h->D.e_cost, h->num_envs, h->cost_ring, h->cost_n);
            HIPCHK(h, hipGetLastError());
            h->cost_n++;
        }
        hipLaunchKernelGGL(k_episode_metrics, dim3((h->num_envs + 255) / 256), dim3(256), 0, st, h->P, h->D, mode == MODE_STEP ? 0 : 1, mask);
        HIPCHK(h, hipGetLastError());
    }
    if (h->timing) HIPCHK(h, hipEventRecord(e1, st));
    if (raster && obs) {
        if (h->P.env_kind == BP_ENV_MAZE)
            hipLaunchKernelGGL(k_observe_maze, dim3(h->num_envs), dim3(OBS_THREADS), h->obs_lds_bytes, st, h->P, h->D, mask, obs);
        else
            hipLaunchKernelGGL(k_observe, dim3(h->num_envs), dim3(OBS_THREADS_SHIP), h->obs_lds_bytes, st, h->P, h->D, mask, obs);
        HIPCHK(h, hipGetLastError());
    }
    if (h->timing) HIPCHK(h, hipEventRecord(e2, st));
    return BP_OK;
}
// Every kernel of one call of the entry points below.  With timing on, the call takes an event triple: e0 here, e1 between physics and observation, e2 at the end.
static int launch(bp_handle *h, int mode, const double *actions, const unsigned char *mask, const StepOut &out, hipStream_t st, bool physics, bool raster,
                  const AsyncArgs *as = nullptr)
{
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (h->timing) {
        if (h->ev_used + 3 > h->ev.size()) {
            for (int k = 0; k < 3; k++) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); h->ev.push_back(e); }
        }
        e0 = h->ev[h->ev_used]; e1 = h->ev[h->ev_used + 1]; e2 = h->ev[h->ev_used + 2];
        h->ev_used += 3;
        HIPCHK(h, hipEventRecord(e0, st));
    }
    if (h->P.env_kind == BP_ENV_BOX) return launch_box(h, mode, actions, mask, out, st, physics, raster, as, e1, e2);
    return launch_rigid(h, mode, actions, mask, out, st, physics, raster, e1, e2);
}
// The reset kernels for the envs of `mask` (null: all).  Resets are not part of the per-step kernel timing.
static int launch_reset_untimed(bp_handle *h, const unsigned char *mask, unsigned char *obs, double *info, hipStream_t st)
{
    const bool save = h->timing;
    h->timing = false;
    const int rc = launch(h, MODE_RESET, nullptr, mask, StepOut{obs, nullptr, nullptr, nullptr, info}, st, true, true);
    h->timing = save;
    return rc;
}

int bp_reset(bp_handle *h, const uint8_t *env_mask, uint8_t *obs, double *info, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "bp_load_scenarios has not been called");
    if (h->q_batch > 0 && env_mask != nullptr)
        return fail(h, BP_ESTATE, "bp_reset with a mask while a ready queue is open: envs are reset through bp_bd_queue_send (bp_bd_queue_close or a reset of all envs closes the queue)");
    BP_DEVICE(h);
    if (h->async_open && env_mask != nullptr) {   // an asynchronous slice is open: the busy envs of the mask are cancelled (a reset of all envs closes the slice instead)
        hipLaunchKernelGGL(k_bd_async_cancel, dim3((h->num_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->Q, env_mask, h->num_envs);
        HIPCHK(h, hipGetLastError());
    }
    const int rc = launch_reset_untimed(h, env_mask, obs, info, (hipStream_t)stream);
    if (rc == BP_OK) h->was_reset = true;
    if (rc == BP_OK && env_mask == nullptr) { h->async_open = false; h->q_batch = 0; }   // (an open ready queue is discarded with the slice)
    return rc;
}

int bp_step(bp_handle *h, const double *actions, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
            double *info, void *stream)
{
    if (!h || !actions) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_step before bp_load_scenarios/bp_reset");
    if (h->async_open) return fail(h, BP_ESTATE, "bp_step while an asynchronous slice is open (bp_bd_async_drain or a reset of all envs closes it)");
    BP_DEVICE(h);
    return launch(h, MODE_STEP, actions, nullptr, StepOut{obs, reward, terminated, truncated, info}, (hipStream_t)stream, true, true);
}

int bp_step_physics(bp_handle *h, const double *actions, double *reward, uint8_t *terminated, uint8_t *truncated, double *info,
                    void *stream)
{
    if (!h || !actions) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_step_physics before bp_load_scenarios/bp_reset");
    if (h->async_open) return fail(h, BP_ESTATE, "bp_step_physics while an asynchronous slice is open (bp_bd_async_drain or a reset of all envs closes it)");
    BP_DEVICE(h);
    return launch(h, MODE_STEP, actions, nullptr, StepOut{nullptr, reward, terminated, truncated, info}, (hipStream_t)stream, true, false);
}

// ---- asynchronous step of box-delivery / area-clearing (DESIGN.md "Asynchronous step") ----
static int async_ready(bp_handle *h, const char *what)
{
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, std::string(what) + " before bp_bd_load / bp_reset");
    if (h->P.env_kind != BP_ENV_BOX || h->Q.unfin == nullptr) return fail(h, BP_EINVAL, std::string(what) + ": not a box-delivery / area-clearing handle (the steps of the other environments have a fixed length)");
    if (h->damp) return fail(h, BP_EINVAL, std::string(what) + ": handles with sim.damping != 0 have no asynchronous step");
    return BP_OK;
}

// Opens the slice, if none is open.  The flag is set before anything of the call is enqueued: should the call fail part-way, envs may already be busy, and the
// handle must refuse bp_step / bp_save_state until a drain or a reset of all envs.
static int slice_open(bp_handle *h, bool clear_unfin, hipStream_t st)
{
    if (!h->async_open) {
        if (clear_unfin) HIPCHK(h, hipMemsetAsync(h->Q.unfin, 0, (size_t)h->num_envs, st));
        if (h->as_epoch > 0x7FFF0000) {   // (serial numbers start over long before they wrap)
            HIPCHK(h, hipMemsetAsync(h->Q.rs_i, 0, sizeof(int) * 16 * (size_t)h->num_envs, st));
            h->as_epoch = 0;
        }
    }
    h->async_open = true;
    return BP_OK;
}
// The drain: the busy envs run to the end of their env steps with no budget; idle envs, and the held ones of a ready queue, emit nothing.
static int launch_drain(bp_handle *h, const StepOut &out, unsigned char *ready, int *slices, hipStream_t st)
{
    const AsyncArgs as = {0, ready, slices};
    return launch(h, MODE_DRAIN, nullptr, nullptr, out, st, true, true, &as);
}

int bp_bd_step_async(bp_handle *h, const double *actions, int32_t budget, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
                     double *info, uint8_t *ready, int32_t *slices, void *stream)
{
    if (!h || !actions || !reward || !terminated || !truncated || !info || !ready || !slices) return BP_EINVAL;
    if (int rc = async_ready(h, "bp_bd_step_async")) return rc;
    if (budget < 1) return fail(h, BP_EINVAL, "bp_bd_step_async: budget < 1 sim step");
    if (h->q_batch > 0) return fail(h, BP_ESTATE, "bp_bd_step_async while a ready queue is open (bp_bd_queue_recv steps the envs; bp_bd_queue_close or a reset of all envs closes it)");
    BP_DEVICE(h);
    // every env is idle on opening.  The lock-step second pass never clears the group byte, and a drain leaves 2 in it: clear
    if (int rc = slice_open(h, true, (hipStream_t)stream)) return rc;
    const AsyncArgs as = {budget, ready, slices};
    return launch(h, MODE_ASYNC, actions, nullptr, StepOut{obs, reward, terminated, truncated, info}, (hipStream_t)stream, true, true, &as);
}

int bp_bd_async_drain(bp_handle *h, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated, double *info, uint8_t *ready,
                      int32_t *slices, void *stream)
{
    if (!h || !reward || !terminated || !truncated || !info || !ready || !slices) return BP_EINVAL;
    if (int rc = async_ready(h, "bp_bd_async_drain")) return rc;
    if (h->q_batch > 0) return fail(h, BP_ESTATE, "bp_bd_async_drain while a ready queue is open (bp_bd_queue_close drains and closes it)");
    BP_DEVICE(h);
    if (!h->async_open) {   // no env is busy: nothing to finish
        HIPCHK(h, hipMemsetAsync(ready, 0, (size_t)h->num_envs, (hipStream_t)stream));
        return BP_OK;
    }
    const int rc = launch_drain(h, StepOut{obs, reward, terminated, truncated, info}, ready, slices, (hipStream_t)stream);
    if (rc == BP_OK) h->async_open = false;
    return rc;
}

int32_t bp_bd_async_open(bp_handle *h) { return (h && h->async_open) ? 1 : 0; }

// ---- ready queue of the asynchronous step (bp_asyncq.hpp; DESIGN.md "Asynchronous step") ----
static int queue_ready(bp_handle *h, const char *what)
{
    if (int rc = async_ready(h, what)) return rc;
    if (h->q_batch < 1) return fail(h, BP_ESTATE, std::string(what) + ": no ready queue is open (bp_bd_queue_open)");
    return BP_OK;
}
static int queue_action_dim(const bp_handle *h) { return h->B.action_type == 2 ? 2 : 1; }

int bp_bd_queue_open(bp_handle *h, int32_t batch, void *stream)
{
    if (!h) return BP_EINVAL;
    if (int rc = async_ready(h, "bp_bd_queue_open")) return rc;
    if (h->async_open) return fail(h, BP_ESTATE, "bp_bd_queue_open while an asynchronous slice is open (bp_bd_async_drain, bp_bd_queue_close or a reset of all envs closes it)");
    const int E = h->num_envs;
    if (batch < 1 || batch > E) return fail(h, BP_EINVAL, "bp_bd_queue_open: batch outside [1, num_envs]");
    BP_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->q.ring == nullptr) {
        BdQueue q = {};
        int rc;
        if ((rc = dalloc(h, &q.hdr, (size_t)4))) return rc;
        if ((rc = dalloc(h, &q.where, (size_t)E))) return rc;
        if ((rc = dalloc(h, &q.fresh, (size_t)E))) return rc;
        if ((rc = dalloc(h, &q.rmask, (size_t)E))) return rc;
        if ((rc = dalloc(h, &q.win, (size_t)E))) return rc;
        if ((rc = dalloc(h, &q.actions, (size_t)E * 2))) return rc;
        if ((rc = dalloc(h, &q.ring, (size_t)E))) return rc;   // last: the queue is allocated once all of it is
        h->q = q;
    }
    HIPCHK(h, hipMemsetAsync(h->q.hdr, 0, sizeof(int) * 4, st));
    HIPCHK(h, hipMemsetAsync(h->q.where, 0, (size_t)E, st));
    HIPCHK(h, hipMemsetAsync(h->q.actions, 0, sizeof(double) * 2 * (size_t)E, st));
    // no clear of the group bytes here: the enqueue kernel below writes every env's (held)
    if (int rc = slice_open(h, false, st)) return rc;
    h->q_batch = batch;
    // every env becomes held and is queued with its current (reset) observation as a fresh row, in env-id order
    hipLaunchKernelGGL(k_bdq_enqueue, dim3(1), dim3(BDQ_THREADS), 0, st, h->q, h->Q.unfin, (const unsigned char *)nullptr, E, 1);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}

int bp_bd_queue_recv(bp_handle *h, int32_t budget, int32_t flags, uint8_t *obs_e, double *reward_e, uint8_t *terminated_e, uint8_t *truncated_e, double *info_e,
                     uint8_t *emitted, int32_t *slices_e, int32_t *ids, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
                     double *info, int32_t *slices, int32_t *counts, void *stream)
{
    if (!h || !reward_e || !terminated_e || !truncated_e || !info_e || !emitted || !slices_e || !ids || !reward || !terminated || !truncated || !info ||
        !slices || !counts)
        return BP_EINVAL;
    if (int rc = queue_ready(h, "bp_bd_queue_recv")) return rc;
    if (budget < 1) return fail(h, BP_EINVAL, "bp_bd_queue_recv: budget < 1 sim step");
    if ((obs == nullptr) != (obs_e == nullptr)) return fail(h, BP_EINVAL, "bp_bd_queue_recv: obs_e and obs must both be given or both be NULL");
    const size_t row = (size_t)h->B.local_px * h->B.local_px * 4;
    if (obs && (row % 16 != 0 || ((uintptr_t)obs_e | (uintptr_t)obs) % 16 != 0))
        return fail(h, BP_EINVAL, "bp_bd_queue_recv: observation rows must be multiples of 16 bytes in 16-byte aligned tensors");
    BP_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    const int E = h->num_envs, M = h->q_batch;
    // 1. one slice call exactly as bp_bd_step_async launches it; the envs take their actions from the queue's action rows (bp_bd_queue_send wrote them)
    const AsyncArgs as = {budget, emitted, slices_e};
    if (int rc = launch(h, MODE_ASYNC, h->q.actions, nullptr, StepOut{obs_e, reward_e, terminated_e, truncated_e, info_e}, st, true, true, &as)) return rc;
    // 2. the envs that emitted are appended in ascending env id and become held; 3. up to M ids leave the head; 4. their rows are gathered
    hipLaunchKernelGGL(k_bdq_enqueue, dim3(1), dim3(BDQ_THREADS), 0, st, h->q, h->Q.unfin, (const unsigned char *)emitted, E, 0);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_bdq_take, dim3(1), dim3(BDQ_THREADS), 0, st, h->q, (const unsigned char *)h->Q.unfin, E, M, (flags & BP_QUEUE_FULL_ONLY) ? 1 : 0, ids, counts);
    HIPCHK(h, hipGetLastError());
    const int row16 = (int)(row / 16);
    hipLaunchKernelGGL(k_bdq_gather, dim3((row16 + BDQ_GATHER_THREADS - 1) / BDQ_GATHER_THREADS, M), dim3(BDQ_GATHER_THREADS), 0, st, (const int *)ids,
                       (const unsigned char *)h->q.fresh, E, (const uint4 *)obs_e, (uint4 *)obs, row16, (const double *)reward_e,
                       (const unsigned char *)terminated_e, (const unsigned char *)truncated_e, (const double *)info_e, (const int *)slices_e, reward,
                       terminated, truncated, info, slices, BP_INFO_COUNT);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}

int bp_bd_queue_send(bp_handle *h, const double *actions, const int32_t *ids, const uint8_t *reset, uint8_t *obs_e, double *info_e, void *stream)
{
    if (!h || !actions || !ids) return BP_EINVAL;
    if (int rc = queue_ready(h, "bp_bd_queue_send")) return rc;
    if (reset != nullptr && !info_e) return fail(h, BP_EINVAL, "bp_bd_queue_send: reset rows need the envs' info rows");
    BP_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    const int E = h->num_envs;
    hipLaunchKernelGGL(k_bdq_send, dim3(1), dim3(BDQ_THREADS), 0, st, h->q, h->Q.unfin, E, h->q_batch, queue_action_dim(h), actions, (const int *)ids, reset);
    HIPCHK(h, hipGetLastError());
    if (reset == nullptr) return BP_OK;
    // the reset rows: the masked reset of bp_reset with the mask the send kernel built (held envs are not busy: nothing to cancel), then their fresh rows
    if (int rc = launch_reset_untimed(h, h->q.rmask, obs_e, info_e, st)) return rc;
    hipLaunchKernelGGL(k_bdq_enqueue, dim3(1), dim3(BDQ_THREADS), 0, st, h->q, h->Q.unfin, (const unsigned char *)h->q.rmask, E, 1);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}

int bp_bd_queue_close(bp_handle *h, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated, double *info, uint8_t *ready, int32_t *slices,
                      void *stream)
{
    if (!h || !reward || !terminated || !truncated || !info || !ready || !slices) return BP_EINVAL;
    if (int rc = queue_ready(h, "bp_bd_queue_close")) return rc;
    BP_DEVICE(h);
    if (int rc = launch_drain(h, StepOut{obs, reward, terminated, truncated, info}, ready, slices, (hipStream_t)stream)) return rc;
    HIPCHK(h, hipMemsetAsync(h->Q.unfin, 0, (size_t)h->num_envs, (hipStream_t)stream));   // every env is idle, the queue is discarded
    h->async_open = false;
    h->q_batch = 0;
    return BP_OK;
}

int32_t bp_bd_queue_batch(bp_handle *h) { return h ? h->q_batch : 0; }

int bp_observe(bp_handle *h, const uint8_t *env_mask, uint8_t *obs, void *stream)
{
    if (!h || !obs) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_observe before bp_load_scenarios/bp_reset");
    BP_DEVICE(h);
    return launch(h, MODE_STEP, nullptr, env_mask, StepOut{obs, nullptr, nullptr, nullptr, nullptr}, (hipStream_t)stream, false, true);
}

int bp_observe_global(bp_handle *h, const uint8_t *env_mask, uint8_t *obs, void *stream)
{
    if (!h || !obs) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_observe_global before bp_load_scenarios/bp_reset");
    if (h->P.env_kind != BP_ENV_SHIP_ICE) return fail(h, BP_ESTATE, "global observation exists for ship-ice only");
    BP_DEVICE(h);
    const int cell_px = (int)(0.2 * h->cfg.m_to_pix); // grid_width 0.2 m (ship_ice_env.py:97), block = int(0.2 * 25) = 5 px
    if (cell_px <= 0 || h->P.grid_h % cell_px || h->P.grid_w % cell_px) return fail(h, BP_EINVAL, "raster is not a multiple of the cell");
    const size_t lds = (size_t)4 * ((h->P.grid_h * h->P.grid_w + 31) / 32);
    HIPCHK(h, hipFuncSetAttribute((const void *)k_observe_global, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_observe_global, dim3(h->num_envs), dim3(OBS_THREADS), lds, (hipStream_t)stream, h->P, h->D, env_mask, obs, cell_px);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}

__global__ void k_export_polys(const DevParams P, const DevPtrs D, double *out, int *counts)
{
    const int env = blockIdx.x;
    const size_t eb = (size_t)env * P.nbcap;
    const int nb = D.e_nb[env];
    const int *nv = D.sc_nv + (size_t)D.e_trial[env] * P.nbcap;
    for (int i = threadIdx.x; i < P.nbcap; i += blockDim.x) {
        const int n = (i < nb) ? nv[i] : 0;
        counts[eb + i] = n;
        for (int q = 0; q < BP_MAXV; q++) {
            const d2 v = (q < n) ? D.wv[(eb + i) * BP_MAXV + q] : mk2(0.0, 0.0);
            out[((eb + i) * BP_MAXV + q) * 2] = v.x;
            out[((eb + i) * BP_MAXV + q) * 2 + 1] = v.y;
        }
    }
}
__global__ void k_export_bodies(const DevParams P, const DevPtrs D, double *out)
{
    const int env = blockIdx.x;
    const size_t eb = (size_t)env * P.nbcap;
    const int nb = D.e_nb[env];
    for (int i = threadIdx.x; i < P.nbcap; i += blockDim.x) {
        double *o = out + (eb + i) * 9;
        if (i < nb) {
            o[0] = D.pxy[eb + i].x; o[1] = D.pxy[eb + i].y; o[2] = D.ang[eb + i];
            o[3] = D.velv[eb + i].x; o[4] = D.velv[eb + i].y; o[5] = D.velw[eb + i].x;
            o[6] = D.velb[eb + i].x; o[7] = D.velb[eb + i].y; o[8] = D.velw[eb + i].y;
        } else {
            for (int k = 0; k < 9; k++) o[k] = 0.0;
        }
    }
}
// generate_observation_low_dim (ship_ice_env.py:358-370): |centroid| of each floe's world polygon
__global__ void k_export_lowdim(const DevParams P, const DevPtrs D, double *out)
{
    const int env = blockIdx.x;
    const size_t eb = (size_t)env * P.nbcap;
    const int nb = D.e_nb[env];
    const int *nv = D.sc_nv + (size_t)D.e_trial[env] * P.nbcap;
    for (int i = 1 + threadIdx.x; i < P.nbcap; i += blockDim.x) {
        double *o = out + ((size_t)env * (P.nbcap - 1) + (i - 1)) * 2;
        if (i < nb) {
            const d2 c = poly_centroid_seq(D.wv + (eb + i) * BP_MAXV, nv[i]);
            o[0] = __builtin_fabs(c.x); o[1] = __builtin_fabs(c.y);
        } else { o[0] = 0.0; o[1] = 0.0; }
    }
}

int bp_get_world_polys(bp_handle *h, double *out, int32_t *counts, void *stream)
{
    if (!h || !out || !counts) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "not reset");
    BP_DEVICE(h);
    hipLaunchKernelGGL(k_export_polys, dim3(h->num_envs), dim3(256), 0, (hipStream_t)stream, h->P, h->D, out, counts);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
double bp_start_uniform(uint64_t seed, int64_t global_env_id, int64_t episode) { return bp_start_u01(seed, global_env_id, episode); }

int bp_get_episode_metrics(bp_handle *h, double *rows, uint32_t *counts, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    if (rows) HIPCHK(h, hipMemcpyAsync(rows, h->D.m_rows, sizeof(double) * BP_EPM_COUNT * h->num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (counts) HIPCHK(h, hipMemcpyAsync(counts, h->D.m_count, sizeof(unsigned) * h->num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BP_OK;
}

int bp_get_episode_history(bp_handle *h, double *ring, double *sums, uint32_t *counts, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    const size_t E = (size_t)h->num_envs;
    if (ring) HIPCHK(h, hipMemcpyAsync(ring, h->D.m_ring, sizeof(double) * BP_EPM_RING * BP_EPM_COUNT * E, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (sums) HIPCHK(h, hipMemcpyAsync(sums, h->D.m_sum, sizeof(double) * BP_EPM_COUNT * E, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (counts) HIPCHK(h, hipMemcpyAsync(counts, h->D.m_count, sizeof(unsigned) * E, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BP_OK;
}

int bp_bd_get_episode_boxes(bp_handle *h, double *out, void *stream)
{
    if (!h || !out) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    if (h->P.env_kind != BP_ENV_BOX) return fail(h, BP_EINVAL, "bp_bd_get_episode_boxes: not a box-delivery / area-clearing handle");
    BP_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(out, h->Q.m_box, sizeof(double) * BD_MAXBOX * 3 * (size_t)h->num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BP_OK;
}

int bp_bd_get_completed(bp_handle *h, uint8_t *out_host)
{
    if (!h || !out_host) return BP_EINVAL;
    if (!h->loaded || h->P.env_kind != BP_ENV_BOX) return fail(h, BP_EINVAL, "bp_bd_get_completed: not a loaded box-delivery / area-clearing handle");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    const size_t n = (size_t)h->num_envs * BD_MAXBOX;
    HIPCHK(h, hipMemcpy(out_host, h->B.task == 1 ? h->Q.cleared : h->Q.alive, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) out_host[i] = (uint8_t)((int)(i % BD_MAXBOX) < h->B.nbox && (out_host[i] != 0) == (h->B.task == 1));
    return BP_OK;
}

// host only: the arithmetic of k_task_metrics' emit path (bp_taskmetric.hpp) on caller-supplied data
int bp_task_metric_row(int32_t nbox, const double *boxes_acxy, const uint8_t *completed, int32_t ngoal, const double *goals_xy, const double *start_xy,
                       double robot_mass, double robot_dist, double total_work, double reward, double steps, double *out6)
{
    if (!boxes_acxy || !completed || !goals_xy || !start_xy || !out6 || nbox < 0 || nbox > BD_MAXBOX || ngoal < 1) return -1;
    tm_row(nbox, boxes_acxy, completed, ngoal, goals_xy, start_xy[0], start_xy[1], robot_mass, robot_dist, total_work, reward, steps, out6);
    return 0;
}

// test hook: every written hint word of the live envs gets random VALID contents -- plane and support-vertex indices below the vertex counts the word
// records, a random subset of the HW_* flags.  The sub-step evaluates cached planes exactly and searches whatever they do not certify, so the results
// of the following steps must not change (tests/test_gpu_parity.py); only the amount of work does.
__global__ __launch_bounds__(256) void k_debug_scramble_hints(unsigned long long *hint, size_t n, unsigned long long seed, int *count)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long hw = hint[i];
    const unsigned nA = (unsigned)HW_NV_A(hw), nB = (unsigned)HW_NV_B(hw);
    if (nA == 0 || nB == 0) return; // never written (or cleared by a neighbour-list refresh)
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1); // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    const unsigned iA = (unsigned)(z & 0xFF) % nA, iB = (unsigned)((z >> 8) & 0xFF) % nB, jA = (unsigned)((z >> 16) & 0xFF) % nB, jB = (unsigned)((z >> 24) & 0xFF) % nA;
    hint[i] = (unsigned long long)(iA | (iB << 5) | (jA << 10) | (jB << 15) | (nA << 20) | (nB << 25)) |
              (((z >> 32) & 1ull) ? HW_HAS_A : 0ull) | (((z >> 33) & 1ull) ? HW_HAS_B : 0ull) | (((z >> 34) & 1ull) ? HW_PRIM_B : 0ull) |
              (((z >> 35) & 1ull) ? HW_BOTH : 0ull);
    atomicAdd(count, 1);
}

int bp_debug_scramble_hints(bp_handle *h, uint64_t seed, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "not reset");
    DevGuard _dg(h->device);
    const size_t n = (size_t)h->num_envs * (size_t)h->nbcap * BP_KADJ;
    int *cnt = nullptr, host = 0;
    HIPCHK(h, hipMalloc(&cnt, sizeof(int)));
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int), (hipStream_t)stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_scramble_hints, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->D.hint, n, (unsigned long long)seed, cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host, cnt, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(cnt);   // also on the error paths
    HIPCHK(h, e);
    return host; // number of hint words rewritten (>= 0; negative = BP_E*)
}

// rows of `src` whose mask byte is set -> the same rows of `dst`; one workgroup per row, 16-byte accesses when the row allows them
__global__ __launch_bounds__(256) void k_copy_rows_masked(const unsigned char *__restrict__ mask, const unsigned *__restrict__ src, unsigned *__restrict__ dst,
                                                          const long long row_words)
{
    const long long r = blockIdx.x;
    if (mask[r] == 0) return;
    const unsigned *s = src + r * row_words;
    unsigned *d = dst + r * row_words;
    if ((row_words & 3) == 0 && ((((size_t)s) | ((size_t)d)) & 15) == 0) {
        const uint4 *s4 = (const uint4 *)s; uint4 *d4 = (uint4 *)d;
        for (long long i = threadIdx.x; i < row_words / 4; i += blockDim.x) d4[i] = s4[i];
    } else
        for (long long i = threadIdx.x; i < row_words; i += blockDim.x) d[i] = s[i];
}

int bp_copy_rows_masked(bp_handle *h, const uint8_t *mask, const void *src, void *dst, int64_t rows, int64_t row_bytes, void *stream)
{
    if (!h || !mask || !src || !dst || rows < 0 || row_bytes <= 0 || (row_bytes & 3) != 0 || rows > 0x7FFFFFFF) return BP_EINVAL;
    if ((((size_t)src) | ((size_t)dst)) & 3) return BP_EINVAL;
    BP_DEVICE(h);
    if (rows == 0) return BP_OK;
    hipLaunchKernelGGL(k_copy_rows_masked, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const unsigned char *)mask, (const unsigned *)src,
                       (unsigned *)dst, (long long)(row_bytes / 4));
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}

int bp_debug_round2(const double *in_dev, double *out_dev, int32_t n, void *stream)
{
    if (!in_dev || !out_dev || n < 0) return BP_EINVAL;
    hipLaunchKernelGGL(k_debug_round2, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, in_dev, out_dev, n);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}

int bp_get_body_state(bp_handle *h, double *out, void *stream)
{
    if (!h || !out) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "not reset");
    BP_DEVICE(h);
    hipLaunchKernelGGL(k_export_bodies, dim3(h->num_envs), dim3(256), 0, (hipStream_t)stream, h->P, h->D, out);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
int bp_costmap_update(bp_handle *h, const bp_costmap_config *cfg, const double *ship_pos_y, double vs, double *out, void *stream)
{
    if (!h || !cfg || !out) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_costmap_update before bp_load_scenarios/bp_reset");
    if (h->P.env_kind != BP_ENV_SHIP_ICE) return fail(h, BP_EINVAL, "bp_costmap_update: ship-ice handles only");
    const int H = (int)(cfg->m * cfg->scale), W = (int)(cfg->n * cfg->scale);
    if (!(cfg->scale > 0) || H <= 0 || W <= 0 || cfg->margin < 0 || 2 * cfg->margin > W) return fail(h, BP_EINVAL, "bp_costmap_update: bad grid");
    BP_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)h->num_envs * H * W;
    const int nblk = (int)std::min<size_t>((total + 255) / 256, 65535);
    hipLaunchKernelGGL(k_costmap_init, dim3(nblk), dim3(256), 0, st, out, h->num_envs, H, W, (int)cfg->margin);
    const int groups = (h->P.nbcap - h->P.nkin + 3) / 4;
    if (groups > 0)
        hipLaunchKernelGGL(k_costmap, dim3(h->num_envs, groups), dim3(256), 0, st, h->P, h->D, cfg->scale, H, W, cfg->alpha, cfg->ship_mass,
                           cfg->horizon > 0 ? cfg->horizon * cfg->scale : 0.0, ship_pos_y, vs, out);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
int32_t bp_sizeof_swath_config(void) { return (int32_t)sizeof(bp_swath_config); }
int bp_swath_cost(bp_handle *h, const bp_swath_config *cfg, const double *cost_maps, const double *paths, const int32_t *lengths, const int32_t *rows,
                  const double *footprint, double *costs, uint8_t *swaths, void *stream)
{
    if (!h || !cfg || !cost_maps || !paths || !footprint || !costs) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_swath_cost before bp_load_scenarios/bp_reset");
    if (h->P.env_kind != BP_ENV_SHIP_ICE) return fail(h, BP_EINVAL, "bp_swath_cost: ship-ice handles only");
    if (cfg->H <= 0 || cfg->W <= 0 || cfg->K <= 0 || cfg->P <= 0) return fail(h, BP_EINVAL, "bp_swath_cost: H, W, K and P must be positive");
    if (cfg->nv < 3 || cfg->nv > BP_MAXV) return fail(h, BP_EINVAL, "bp_swath_cost: footprint of 3 .. 20 vertices");
    if (cfg->outside != BP_SWATH_CLIP && cfg->outside != BP_SWATH_REJECT) return fail(h, BP_EINVAL, "bp_swath_cost: unknown outside mode");
    const long long WW = ((long long)cfg->W + 63) / 64, words = (long long)cfg->H * WW;
    if (words > BP_SWATH_MAX_WORDS) return fail(h, BP_EINVAL, "bp_swath_cost: grid above the LDS limit (H * ceil(W / 64) <= 4096)");
    const long long cells = (long long)cfg->H * cfg->W, ncand = (long long)h->num_envs * cfg->K;
    if (cfg->map_stride < 0 || (cfg->map_stride > 0 && cfg->map_stride < cells)) return fail(h, BP_EINVAL, "bp_swath_cost: bad map_stride");
    if (ncand > 0x7FFFFFFFll || (long long)cfg->P * 3 > 0x7FFFFFFFll) return fail(h, BP_EINVAL, "bp_swath_cost: too many candidates or samples");
    BP_DEVICE(h);
    SwathArgs A;
    A.H = cfg->H; A.W = cfg->W; A.K = cfg->K; A.P = cfg->P; A.nv = cfg->nv; A.WW = (int)WW; A.outside = cfg->outside;
    A.vec4 = swaths && (((uintptr_t)swaths) & 3u) == 0 && (cells & 3) == 0;
    A.map_stride = cfg->map_stride;
    A.maps = cost_maps; A.paths = paths; A.fp = footprint; A.lengths = lengths; A.rows = rows; A.costs = costs; A.swaths = swaths;
    hipLaunchKernelGGL(k_swath_cost, dim3((unsigned)ncand), dim3(64), (size_t)words * 8, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
// ---- path tracking ----
int32_t bp_sizeof_track_config(void) { return (int32_t)sizeof(bp_track_config); }
int bp_track_path(bp_handle *h, const bp_track_config *cfg, const double *paths, int64_t path_stride, const int32_t *lengths, const double *poses,
                  const uint8_t *active, double *state, double *actions, double *ct_err, int32_t *diag, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!cfg || !paths || !poses || !state || !actions || !ct_err) return fail(h, BP_EINVAL, "bp_track_path: NULL required pointer");
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_track_path before bp_load_scenarios/bp_reset");
    if (h->P.env_kind != BP_ENV_SHIP_ICE) return fail(h, BP_EINVAL, "bp_track_path: ship-ice handles only");
    if (cfg->P <= 0 || (long long)cfg->P * 3 > 0x7FFFFFFFll) return fail(h, BP_EINVAL, "bp_track_path: P must be positive (and 3 * P below 2^31)");
    if (path_stride < 0 || (path_stride > 0 && path_stride < 3ll * cfg->P)) return fail(h, BP_EINVAL, "bp_track_path: bad path_stride");
    if (!(cfg->dt > 0.0) || !std::isfinite(cfg->dt) || !(cfg->action_scale > 0.0) || !std::isfinite(cfg->action_scale))
        return fail(h, BP_EINVAL, "bp_track_path: dt and action_scale must be positive and finite");
    BP_DEVICE(h);
    TrackArgs A;
    A.c = *cfg; A.path_stride = path_stride; A.paths = paths; A.poses = poses; A.lengths = lengths; A.active = active;
    A.state = state; A.actions = actions; A.ct_err = ct_err; A.diag = diag;
    hipLaunchKernelGGL(k_track_path, dim3((unsigned)h->num_envs), dim3(64), 0, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
// ---- batched RRT and the waypoint controller ----
int32_t bp_sizeof_rrt_config(void) { return (int32_t)sizeof(bp_rrt_config); }
int32_t bp_sizeof_track_wp_config(void) { return (int32_t)sizeof(bp_track_wp_config); }
double bp_rrt_uniform(uint64_t seed, int64_t stream, int32_t pass, int32_t iteration, int32_t draw)
{
    return bp_rrt_u01(seed, stream, pass, iteration, draw);
}
static const char *rrt_config_error(const bp_rrt_config *c)
{
    const double v[6] = {c->step, c->goal_radius, c->goal_bias, c->densify_ds, c->prune_min_dist, c->inflate_radius};
    for (double x : v) if (!std::isfinite(x) || x < 0.0) return "bp_rrt_plan: a config value is negative or not finite";
    if (!(c->step > 0.0)) return "bp_rrt_plan: step must be positive";
    if (c->max_nodes < 1 || c->max_nodes > 0x3FFFFFFF) return "bp_rrt_plan: max_nodes must be 1 .. 2^30 - 1";
    if (c->max_waypoints < 2 || c->max_waypoints > 0x3FFFFFFF) return "bp_rrt_plan: max_waypoints must be at least 2";
    if (c->passes < 1 || c->passes > 2) return "bp_rrt_plan: passes must be 1 or 2";
    if (!(((double)c->max_nodes + 2.0) * std::fmax(1.0, std::fmax(c->step, c->goal_radius) / std::fmax(1e-3, c->densify_ds)) <= RRT_DENSE_POINTS_MAX))
        return "bp_rrt_plan: (max_nodes + 2) * max(1, max(step, goal_radius) / max(1e-3, densify_ds)) exceeds 2^22 dense points";
    return nullptr;
}
static long long rrt_per_env(const bp_rrt_config *c) { return (((long long)c->max_nodes + 2) * 20 + 15) & ~15ll; }
int64_t bp_rrt_workspace_bytes(const bp_rrt_config *cfg, int32_t num_envs)
{
    if (!cfg || num_envs <= 0 || rrt_config_error(cfg)) return BP_EINVAL;
    return (int64_t)(rrt_per_env(cfg) * num_envs);
}
int bp_rrt_plan(bp_handle *h, const bp_rrt_config *cfg, const double *starts, const double *goals, const double *walls, int32_t n_walls,
                const double *boxes, const int32_t *counts, int32_t n_boxes, int32_t n_verts, const int64_t *streams, const uint8_t *active,
                void *workspace, int64_t workspace_bytes, int32_t *status, int32_t *n_nodes, int32_t *iterations, double *paths, int32_t *lengths,
                void *stream)
{
    if (!h) return BP_EINVAL;
    if (!cfg || !starts || !goals || !streams || !workspace || !status || !n_nodes || !iterations || !paths || !lengths)
        return fail(h, BP_EINVAL, "bp_rrt_plan: NULL required pointer");
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_rrt_plan before bp_load_maze/bp_reset");
    if (h->P.env_kind != BP_ENV_MAZE) return fail(h, BP_EINVAL, "bp_rrt_plan: maze handles only");
    if (const char *e = rrt_config_error(cfg)) return fail(h, BP_EINVAL, e);
    if (n_walls < 0 || n_walls > BP_RRT_MAX_WALLS || (n_walls > 0 && !walls)) return fail(h, BP_EINVAL, "bp_rrt_plan: n_walls outside 0 .. BP_RRT_MAX_WALLS");
    if (n_boxes < 0 || (n_boxes > 0 && (n_verts < 3 || n_verts > BP_MAXV || !boxes || !counts)) || (long long)n_boxes * n_verts > BP_RRT_MAX_BOX_VERTS)
        return fail(h, BP_EINVAL, "bp_rrt_plan: n_verts outside 3 .. BP_MAXV or n_boxes * n_verts above BP_RRT_MAX_BOX_VERTS");
    const long long per_env = rrt_per_env(cfg);
    if (workspace_bytes < per_env * (long long)h->num_envs || (((uintptr_t)workspace) & 15u))
        return fail(h, BP_EINVAL, "bp_rrt_plan: workspace smaller than bp_rrt_workspace_bytes or not 16-byte aligned");
    BP_DEVICE(h);
    RrtArgs A;
    A.c = *cfg; A.W = n_walls; A.B = n_boxes; A.V = n_boxes > 0 ? n_verts : 0; A.ws_per_env = per_env;
    A.starts = starts; A.goals = goals; A.walls = walls; A.boxes = boxes; A.counts = counts; A.streams = (const long long *)streams; A.active = active;
    A.ws = (char *)workspace; A.status = status; A.n_nodes = n_nodes; A.iterations = iterations; A.lengths = lengths; A.paths = paths;
    // BP_RRT_LDS_NODES (read at every call; default RRT_LDS_NODES_DEFAULT) is how many of the tree's first nodes the nearest search keeps in LDS: a
    // multiple of 64, at most 2048, 0 for none.  It changes the time of a launch, not the plan (profiles/rrt/README.md)
    int lds_nodes = RRT_LDS_NODES_DEFAULT;
    if (const char *e = getenv("BP_RRT_LDS_NODES")) lds_nodes = atoi(e);
    lds_nodes = lds_nodes < 0 ? 0 : (lds_nodes > 2048 ? 2048 : lds_nodes & ~63);
    lds_nodes = std::min(lds_nodes, (cfg->max_nodes + 2 + 63) & ~63);
    const size_t lds_scene = (size_t)(A.W + A.B * A.V) * 32 + (size_t)(A.B + (A.B & 1)) * 8;     // at most 45056 + 3416 bytes
    lds_nodes = std::min(lds_nodes, (int)((65536 - lds_scene) / 16) & ~63);                       // 64 KB of LDS per workgroup at most
    A.lds_nodes = lds_nodes;
    const size_t lds = lds_scene + (size_t)lds_nodes * 16;
    hipLaunchKernelGGL(k_rrt_plan, dim3((unsigned)h->num_envs), dim3(64), lds, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
int bp_track_waypoints(bp_handle *h, const bp_track_wp_config *cfg, const double *paths, const int32_t *lengths, const double *poses,
                       const uint8_t *active, double *actions, int32_t *diag, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!cfg || !paths || !poses || !actions || !diag) return fail(h, BP_EINVAL, "bp_track_waypoints: NULL required pointer");
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_track_waypoints before bp_load_maze/bp_reset");
    if (h->P.env_kind != BP_ENV_MAZE) return fail(h, BP_EINVAL, "bp_track_waypoints: maze handles only");
    if (cfg->P <= 0 || (long long)cfg->P * 2 > 0x7FFFFFFFll) return fail(h, BP_EINVAL, "bp_track_waypoints: P must be positive (and 2 * P below 2^31)");
    if (!std::isfinite(cfg->Lfc) || !(cfg->dt > 0.0) || !std::isfinite(cfg->dt) || !(cfg->action_scale > 0.0) || !std::isfinite(cfg->action_scale))
        return fail(h, BP_EINVAL, "bp_track_waypoints: Lfc must be finite, dt and action_scale positive and finite");
    BP_DEVICE(h);
    TrackWpArgs A;
    A.c = *cfg; A.paths = paths; A.lengths = lengths; A.poses = poses; A.active = active; A.actions = actions; A.diag = diag;
    hipLaunchKernelGGL(k_track_waypoints, dim3((unsigned)h->num_envs), dim3(64), 0, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
// ---- the GTSP push planner and its controller ----
int32_t bp_sizeof_gtsp_config(void) { return (int32_t)sizeof(bp_gtsp_config); }
static const char *gtsp_config_error(const bp_gtsp_config *c)
{
    const double v[8] = {c->shrink, c->extend, c->lin_vel, c->ang_vel, c->Lfc, c->target_speed, c->switch_dist, 0.0};
    for (double x : v) if (!std::isfinite(x) || x < 0.0) return "bp_gtsp: a config value is negative or not finite";
    if (!(c->dt > 0.0) || !std::isfinite(c->dt) || !(c->v_scale > 0.0) || !std::isfinite(c->v_scale) || !(c->w_scale > 0.0) || !std::isfinite(c->w_scale))
        return "bp_gtsp: dt, v_scale and w_scale must be positive and finite";
    if (c->max_boxes < 1 || c->max_boxes > BP_GTSP_MAX_BOXES) return "bp_gtsp: max_boxes outside 1 .. BP_GTSP_MAX_BOXES";
    if (c->num_goals < 1 || c->num_goals > BP_GTSP_MAX_GOALS) return "bp_gtsp: num_goals outside 1 .. BP_GTSP_MAX_GOALS";
    if (c->round_decimals < 0 || c->round_decimals > 15) return "bp_gtsp: round_decimals outside 0 .. 15";
    return nullptr;
}
static long long gtsp_per_env(const bp_gtsp_config *c) { return (((1ll << c->max_boxes) * c->max_boxes * c->num_goals * 4) + 15) & ~15ll; }
int64_t bp_gtsp_workspace_bytes(const bp_gtsp_config *cfg, int32_t num_envs)
{
    if (!cfg || num_envs <= 0 || gtsp_config_error(cfg)) return BP_EINVAL;
    return (int64_t)(gtsp_per_env(cfg) * num_envs);
}
static bool gtsp_handle(const bp_handle *h) { return h->P.env_kind == BP_ENV_BOX && h->bdcfg.task == 1; }
int bp_gtsp_plan(bp_handle *h, const bp_gtsp_config *cfg, const double *poses, const double *boxes, const int32_t *counts, int32_t n_boxes,
                 int32_t n_verts, const double *goals, const uint8_t *active, void *workspace, int64_t workspace_bytes, int32_t *status,
                 int32_t *n_push, int32_t *tour, int32_t *cost, double *paths, int32_t *lengths, int32_t *track_id, double *track_setpoint,
                 int32_t *weights, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!cfg || !poses || !goals || !workspace || !status || !n_push || !tour || !cost || !paths || !lengths || !track_id || !track_setpoint)
        return fail(h, BP_EINVAL, "bp_gtsp_plan: NULL required pointer");
    if (!gtsp_handle(h)) return fail(h, BP_EINVAL, "bp_gtsp_plan: area-clearing handles only");
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_gtsp_plan before bp_bd_load/bp_reset");
    if (const char *e = gtsp_config_error(cfg)) return fail(h, BP_EINVAL, e);
    if (n_boxes < 0 || n_boxes > BP_GTSP_MAX_SLOTS || (n_boxes > 0 && (n_verts < 3 || n_verts > BP_MAXV || !boxes || !counts)))
        return fail(h, BP_EINVAL, "bp_gtsp_plan: n_boxes above BP_GTSP_MAX_SLOTS or n_verts outside 3 .. BP_MAXV");
    const bp_bd_config &bc = h->bdcfg;
    if (bc.num_boundary_verts < 3 || bc.num_boundary_verts > 8) return fail(h, BP_EINVAL, "bp_gtsp_plan: the handle has no boundary polygon");
    const long long per_env = gtsp_per_env(cfg);
    if (workspace_bytes < per_env * (long long)h->num_envs || (((uintptr_t)workspace) & 15u))
        return fail(h, BP_EINVAL, "bp_gtsp_plan: workspace smaller than bp_gtsp_workspace_bytes or not 16-byte aligned");
    BP_DEVICE(h);
    GtspArgs A;
    A.c = *cfg;
    A.round_scale = 1.0;
    for (int i = 0; i < cfg->round_decimals; i++) A.round_scale *= 10.0;       // exact up to 10^22
    A.B = n_boxes; A.V = n_boxes > 0 ? n_verts : 0; A.G = cfg->num_goals; A.nb = bc.num_boundary_verts;
    A.n_max = cfg->max_boxes; A.N_max = cfg->max_boxes * cfg->num_goals + 1; A.ws_per_env = per_env;
    for (int i = 0; i < 8; i++) { A.boundary[i][0] = bc.boundary[i][0]; A.boundary[i][1] = bc.boundary[i][1]; }
    A.poses = poses; A.boxes = boxes; A.goals = goals; A.counts = counts; A.active = active; A.ws = (char *)workspace;
    A.status = status; A.n_push = n_push; A.tour = tour; A.cost = cost; A.lengths = lengths; A.track_id = track_id; A.W = weights;
    A.paths = paths; A.track_sp = track_setpoint;
    const size_t lds = (((size_t)A.N_max * A.N_max + 3) / 4 + (size_t)A.n_max * A.G * 3 + 2 * (size_t)A.n_max + 1) * 16;   // 42.6 KB at the caps
    hipLaunchKernelGGL(k_gtsp_plan, dim3((unsigned)h->num_envs), dim3(64), lds, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
int bp_gtsp_track(bp_handle *h, const bp_gtsp_config *cfg, const double *paths, const int32_t *lengths, const double *poses, const uint8_t *active,
                  int32_t *track_id, double *track_setpoint, double *actions, int32_t *diag, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!cfg || !paths || !lengths || !poses || !track_id || !track_setpoint || !actions || !diag)
        return fail(h, BP_EINVAL, "bp_gtsp_track: NULL required pointer");
    if (!gtsp_handle(h)) return fail(h, BP_EINVAL, "bp_gtsp_track: area-clearing handles only");
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_gtsp_track before bp_bd_load/bp_reset");
    if (const char *e = gtsp_config_error(cfg)) return fail(h, BP_EINVAL, e);
    BP_DEVICE(h);
    GtspTrackArgs A;
    A.c = *cfg; A.P = 2 * cfg->max_boxes + 1; A.paths = paths; A.poses = poses; A.lengths = lengths; A.active = active;
    A.track_id = track_id; A.diag = diag; A.track_sp = track_setpoint; A.actions = actions;
    hipLaunchKernelGGL(k_gtsp_track, dim3((unsigned)h->num_envs), dim3(64), 0, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
// ---- lattice A* ----
struct LatLayout { long long hcap, off_nodes, off_heap, per_env; };
static bool lattice_layout(const bp_lattice_config *c, LatLayout &L)
{
    if (!c || c->node_capacity <= 0 || c->queue_capacity <= 0 || c->node_capacity > (1 << 24) || c->queue_capacity > (1 << 26)) return false;
    long long hc = 64;
    while (hc < 2ll * c->node_capacity) hc <<= 1;
    L.hcap = hc;
    L.off_nodes = hc * 4;
    L.off_heap = (L.off_nodes + (long long)c->node_capacity * (long long)sizeof(LatNode) + 15) & ~15ll;
    L.per_env = L.off_heap + (long long)c->queue_capacity * (long long)sizeof(LatEntry);
    return true;
}
int32_t bp_sizeof_lattice_config(void) { return (int32_t)sizeof(bp_lattice_config); }
int64_t bp_lattice_workspace_bytes(const bp_lattice_config *cfg, int32_t num_envs)
{
    LatLayout L;
    if (num_envs <= 0 || !lattice_layout(cfg, L)) return BP_EINVAL;
    return (int64_t)(L.per_env * num_envs);
}
int bp_lattice_search(bp_handle *h, const bp_lattice_config *cfg, const double *cost_maps, const double *starts, const double *goal_y, const uint8_t *active,
                      const double *edges_host, const int32_t *edge_headings_host, const double *edge_lengths_host, const int32_t *edge_counts_host,
                      const uint64_t *masks, void *workspace, int64_t workspace_bytes, int32_t *status, double *g, int32_t *expanded, int32_t *n_nodes,
                      double *nodes, int32_t *edges, void *stream)
{
    if (!h || !cfg || !cost_maps || !starts || !goal_y || !edges_host || !edge_headings_host || !edge_lengths_host || !edge_counts_host || !masks ||
        !workspace || !status || !g || !expanded || !n_nodes || !nodes || !edges) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "bp_lattice_search before bp_load_scenarios/bp_reset");
    if (h->P.env_kind != BP_ENV_SHIP_ICE) return fail(h, BP_EINVAL, "bp_lattice_search: ship-ice handles only");
    if (cfg->H <= 0 || cfg->W <= 0) return fail(h, BP_EINVAL, "bp_lattice_search: H and W must be positive");
    if (cfg->S <= 0 || cfg->S > 64 || (cfg->S & 1) == 0) return fail(h, BP_EINVAL, "bp_lattice_search: mask side S must be odd and at most 64 (one mask row per lane)");
    if ((cfg->nh != 8 && cfg->nh != 16) || cfg->nb * 4 != cfg->nh) return fail(h, BP_EINVAL, "bp_lattice_search: 8 or 16 headings, nb = nh / 4");
    if (cfg->ne_max <= 0 || cfg->ne_max > BP_LAT_MAX_EDGES) return fail(h, BP_EINVAL, "bp_lattice_search: 1 .. 32 edges per base heading");
    if (cfg->den <= 0 || cfg->den > 64 || !(cfg->unit > 0.0) || !std::isfinite(cfg->unit) || cfg->margin < 0 || !std::isfinite(cfg->weight) ||
        !(cfg->turning_radius > 0.0) || !std::isfinite(cfg->turning_radius))
        return fail(h, BP_EINVAL, "bp_lattice_search: den, unit, margin, weight or turning_radius out of range");
    if (cfg->max_expansions <= 0 || cfg->node_capacity <= 0 || cfg->queue_capacity <= 0 || cfg->max_path_nodes <= 0)
        return fail(h, BP_EINVAL, "bp_lattice_search: the caps must be positive");
    LatLayout L;
    if (!lattice_layout(cfg, L)) return fail(h, BP_EINVAL, "bp_lattice_search: node_capacity above 2^24 or queue_capacity above 2^26");
    const long long cells = (long long)cfg->H * cfg->W, mwords = (long long)cfg->nh * cfg->ne_max * cfg->S;
    if (cfg->map_stride < 0 || (cfg->map_stride > 0 && cfg->map_stride < cells)) return fail(h, BP_EINVAL, "bp_lattice_search: bad map_stride");
    if (cfg->mask_stride < 0 || (cfg->mask_stride > 0 && cfg->mask_stride < mwords)) return fail(h, BP_EINVAL, "bp_lattice_search: bad mask_stride");
    const double u = cfg->unit / (double)cfg->den;
    if (!(std::hypot((double)cfg->H, (double)cfg->W) / u < (double)(BP_LAT_KEY_OFF - 2)))
        return fail(h, BP_EINVAL, "bp_lattice_search: the map's diagonal exceeds 4094 sub-units");
    if (workspace_bytes < L.per_env * (long long)h->num_envs || (((uintptr_t)workspace) & 15u))
        return fail(h, BP_EINVAL, "bp_lattice_search: workspace smaller than bp_lattice_workspace_bytes or not 16-byte aligned");
    LatticeArgs A;
    memset(&A, 0, sizeof(A));
    for (int b = 0; b < cfg->nb; b++) {
        const int ne = edge_counts_host[b];
        if (ne <= 0 || ne > cfg->ne_max) return fail(h, BP_EINVAL, "bp_lattice_search: edge count outside 1 .. ne_max");
        A.ne[b] = ne;
        for (int k = 0; k < ne; k++) {
            const size_t s = (size_t)b * cfg->ne_max + k;
            const int t = b * BP_LAT_MAX_EDGES + k;
            const double ex = edges_host[2 * s] * cfg->den, ey = edges_host[2 * s + 1] * cfg->den;
            if (!(std::fabs(ex) <= 1024.0 && std::fabs(ey) <= 1024.0) || ex != std::nearbyint(ex) || ey != std::nearbyint(ey))
                return fail(h, BP_EINVAL, "bp_lattice_search: an edge is not a multiple of the sub-unit (unit / den)");
            if (edge_headings_host[s] < 0 || edge_headings_host[s] >= cfg->nh) return fail(h, BP_EINVAL, "bp_lattice_search: edge heading outside [0, nh)");
            A.ex[t] = (short)ex; A.ey[t] = (short)ey; A.eh[t] = (signed char)edge_headings_host[s]; A.len[t] = edge_lengths_host[s];
        }
    }
    BP_DEVICE(h);
    A.H = cfg->H; A.W = cfg->W; A.S = cfg->S; A.mv = cfg->S / 2; A.nh = cfg->nh; A.nb = cfg->nb; A.ne_max = cfg->ne_max; A.margin = cfg->margin;
    A.h_baseline = cfg->h_baseline != 0; A.max_exp = cfg->max_expansions; A.ncap = cfg->node_capacity; A.hcap = (int)L.hcap; A.qcap = cfg->queue_capacity;
    A.nmax = cfg->max_path_nodes; A.map_stride = cfg->map_stride; A.mask_stride = cfg->mask_stride;
    A.ws_stride = (unsigned long long)L.per_env; A.off_nodes = (unsigned long long)L.off_nodes; A.off_heap = (unsigned long long)L.off_heap;
    A.u = u; A.weight = cfg->weight; A.r = cfg->turning_radius;
    A.maps = cost_maps; A.starts = starts; A.goal_y = goal_y; A.active = active; A.masks = (const unsigned long long *)masks; A.ws = (unsigned char *)workspace;
    A.status = status; A.expanded = expanded; A.n_nodes = n_nodes; A.edges = edges; A.g = g; A.nodes = nodes;
    hipLaunchKernelGGL(k_lattice_search, dim3((unsigned)h->num_envs), dim3(64), 0, (hipStream_t)stream, A);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}
int bp_get_low_dim_obs(bp_handle *h, double *out, void *stream)
{
    if (!h || !out) return BP_EINVAL;
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "not reset");
    BP_DEVICE(h);
    hipLaunchKernelGGL(k_export_lowdim, dim3(h->num_envs), dim3(256), 0, (hipStream_t)stream, h->P, h->D, out);
    HIPCHK(h, hipGetLastError());
    return BP_OK;
}

int32_t bp_nb_cap(const bp_handle *h) { return h ? h->nbcap : 0; }
int32_t bp_obs_height(const bp_handle *h) { return h ? h->P.obs_h : 0; }
int32_t bp_obs_width(const bp_handle *h) { return h ? h->P.obs_w : 0; }

// ---- box-delivery-v0 ---------------------------------------------------------------------------------------------------
int32_t bp_bd_sizeof_config(void) { return (int32_t)sizeof(bp_bd_config); }

int bp_bd_create(const bp_bd_config *cfg, int32_t num_envs, int64_t env_id_offset, int32_t device, bp_handle **out)
{
    if (!cfg || !out || num_envs <= 0) return BP_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BP_ENODEVICE;
    if (!(cfg->damping_pow >= 0.0) || cfg->damping_pow > 1.0 || cfg->steps <= 0 || cfg->iterations <= 0 || cfg->persistence <= 0) return BP_EINVAL;
    if (cfg->num_boxes <= 0 || cfg->num_boxes > BD_MAXBOX || cfg->local_px <= 0 || (cfg->local_px & 1)) return BP_EINVAL;
    bp_handle *h = new bp_handle();
    memset(&h->cfg, 0, sizeof(h->cfg));
    h->bdcfg = *cfg;
    h->num_envs = num_envs; h->env_offset = env_id_offset; h->device = device;
    DevGuard _dg(device);
    if (!_dg.ok) { delete h; return BP_ENODEVICE; }
    memset(&h->D, 0, sizeof(h->D));
    memset(&h->Q, 0, sizeof(h->Q));
    DevParams &P = h->P;
    memset(&P, 0, sizeof(P));
    P.dt_sub = cfg->ctrl_dt / cfg->steps;
    P.steps = cfg->steps; P.iterations = cfg->iterations; P.persistence = cfg->persistence; P.settle_steps = cfg->settle_steps;
    if (const char *evp = getenv("BP_DEBUG_PATHS")) P.dbg_paths = atoi(evp); // test hook: force the rarely taken paths of the narrow phase (bp_device.hpp)
    P.bias_lanes = getenv("BP_BIAS_LANES") ? (atoi(getenv("BP_BIAS_LANES")) != 0) : 1;   // 0: sub-steps with a bias term take the bias copy of the solver passes
    P.damping_pow = cfg->damping_pow; P.bias_coef = cfg->bias_coef; P.slop = cfg->slop;
    P.target_speed = cfg->target_speed;
    P.skin = 0.25;
    P.env_kind = BP_ENV_BOX;
    P.nkin = 6;                                            // main shape + 4 wheels + front bumper on one KINEMATIC body
    P.num_envs = num_envs; P.env_offset = env_id_offset;
    P.obs_h = P.obs_w = cfg->local_px;
    BdParams &B = h->B;
    memset(&B, 0, sizeof(B));
    B.room_length = cfg->room_length; B.room_width = cfg->room_width; B.recept_x = cfg->recept_x; B.recept_y = cfg->recept_y;
    B.recept_size = cfg->recept_size; B.ppm = cfg->ppm; B.local_w = cfg->local_w; B.robot_radius = cfg->robot_radius;
    B.step_size = cfg->step_size; B.target_speed = cfg->target_speed; B.ctrl_dt = cfg->ctrl_dt;
    B.partial_rewards_scale = cfg->partial_rewards_scale; B.goal_reward = cfg->goal_reward; B.collision_penalty = cfg->collision_penalty;
    B.non_movement_penalty = cfg->non_movement_penalty; B.correct_direction_reward_scale = cfg->correct_direction_reward_scale;
    B.ministep_size = cfg->ministep_size; B.sp_channel_scale = cfg->sp_channel_scale;
    B.local_px = cfg->local_px; B.use_correct_direction_reward = cfg->use_correct_direction_reward;
    B.inactivity_cutoff = cfg->inactivity_cutoff; B.num_boxes = cfg->num_boxes; B.step_limit = cfg->step_limit;
    B.first_box = 6;
    B.robot_mass = cfg->robot_mass;
    B.action_type = cfg->action_type;
    if (cfg->action_type < 0 || cfg->action_type > 2) { delete h; return BP_EINVAL; }
    B.task = cfg->task; B.omega_scale = cfg->omega_scale; B.v_scale = cfg->v_scale; B.lfc = cfg->lfc;
    B.yaw_rate_step = cfg->yaw_rate_step; B.t_max = cfg->t_max;
    B.boundary_penalty = cfg->boundary_penalty; B.box_cleared_reward = cfg->box_cleared_reward; B.box_putback_penalty = cfg->box_putback_penalty;
    B.truncation_penalty = cfg->truncation_penalty; B.terminal_reward = cfg->terminal_reward; B.pushing_mult = cfg->pushing_mult;
    // outside the small-map window every cell is padding obstacle: spfa leaves 0 there, the inverted map (box_delivery_env.py:1126-1128) 0 + 1
    B.recept_outside = (cfg->task == 0 && cfg->invert_receptacle_map) ? 1.0f : 0.0f;
    if (cfg->task == 1) {
        if (cfg->num_boundary_verts < 3 || cfg->num_boundary_verts > 8 || cfg->num_outer_verts < 3 || cfg->num_outer_verts > 8 ||
            cfg->num_goal_points < 1 || cfg->num_goal_points > 128) { delete h; return BP_EINVAL; }
        B.nbd = cfg->num_boundary_verts; B.nob = cfg->num_outer_verts; B.ngoal = cfg->num_goal_points;
        memcpy(B.bd_poly, cfg->boundary, sizeof(B.bd_poly)); memcpy(B.ob_poly, cfg->outer_boundary, sizeof(B.ob_poly));
        memcpy(B.footprint, cfg->footprint_verts, sizeof(B.footprint));
        B.recept_outside = 1.0f;
    } else if (cfg->task != 0) { delete h; return BP_EINVAL; }
    *out = h;
    return BP_OK;
}

// ---- the box-delivery / area-clearing loader behind upload_trials(), as a sequence of steps -----------------------------------------------------------
// (NW: cells of the small-map window, words: its bitmap words)
// Step 1: the static maps of every distinct layout, the receptacle polygons and the robot channel to the device; their part of the scenario hash
static int bd_upload_maps(bp_handle *h, const bpgeom::BdScene &sc, int NW, int words)
{
    const int T = (int)sc.map_of_trial.size(), nm = (int)sc.maps.size();
    const bool recept = h->bdcfg.task == 0;
    int rc;
    int *d_mot; unsigned *d_free, *d_thin; unsigned short *d_edt; float *d_rec; unsigned char *d_small, *d_rchan; d2 *d_rp, *d_rn;
    if ((rc = dalloc(h, &d_mot, T))) return rc;
    if ((rc = dalloc(h, &d_free, (size_t)nm * words))) return rc;
    if ((rc = dalloc(h, &d_thin, (size_t)nm * words))) return rc;
    if ((rc = dalloc(h, &d_edt, (size_t)nm * NW * 2))) return rc;
    if ((rc = dalloc(h, &d_rec, (size_t)nm * NW))) return rc;
    if ((rc = dalloc(h, &d_small, (size_t)nm * NW))) return rc;
    if ((rc = dalloc(h, &d_rp, (size_t)nm * 4))) return rc;
    if ((rc = dalloc(h, &d_rn, (size_t)nm * 4))) return rc;
    if ((rc = dalloc(h, &d_rchan, sc.robot_chan.size()))) return rc;
    HIPCHK(h, hipMemcpy(d_mot, sc.map_of_trial.data(), sizeof(int) * T, hipMemcpyHostToDevice));
    for (int m = 0; m < nm; m++) {
        const bpgeom::BdMaps &M = sc.maps[m];
        HIPCHK(h, hipMemcpy(d_free + (size_t)m * words, M.free_bits.data(), sizeof(unsigned) * words, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d_thin + (size_t)m * words, M.thin_bits.data(), sizeof(unsigned) * words, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d_edt + (size_t)m * NW * 2, M.edt.data(), sizeof(unsigned short) * NW * 2, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d_rec + (size_t)m * NW, M.recept.data(), sizeof(float) * NW, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d_small + (size_t)m * NW, M.small_free.data(), NW, hipMemcpyHostToDevice));
        if (recept) {
            HIPCHK(h, hipMemcpy(d_rp + (size_t)m * 4, &sc.recept_poly[4 * (size_t)m], sizeof(d2) * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d_rn + (size_t)m * 4, &sc.recept_n[4 * (size_t)m], sizeof(d2) * 4, hipMemcpyHostToDevice));
        }
    }
    HIPCHK(h, hipMemcpy(d_rchan, sc.robot_chan.data(), sc.robot_chan.size(), hipMemcpyHostToDevice));
    BdPtrs &Q = h->Q;
    Q.map_of_trial = d_mot; Q.free_bits = d_free; Q.thin_bits = d_thin; Q.edt = d_edt; Q.recept = d_rec; Q.small_free = d_small;
    Q.recept_poly = d_rp; Q.recept_n = d_rn; Q.robot_chan = d_rchan;
    h->scen_hash = bpgeom::bd_scene_hash(sc, h->scen_hash);
    return BP_OK;
}
// Step 2: the task state of the E envs plus T templates, next to alloc_env_state's
static int bd_alloc_env_state(bp_handle *h, int T, int NW)
{
    const bp_bd_config &cf = h->bdcfg;
    BdPtrs &Q = h->Q;
    int rc;
    const size_t E = (size_t)h->num_envs + (size_t)T;
    if ((rc = dalloc(h, &Q.alive, E * BD_MAXBOX))) return rc;
    if ((rc = dalloc(h, &Q.order, E * BD_MAXBOX))) return rc;
    if ((rc = dalloc(h, &Q.nalive, E))) return rc;
    if ((rc = dalloc(h, &Q.nprev, E))) return rc;
    if ((rc = dalloc(h, &Q.boxdist, E * BD_MAXBOX))) return rc;
    if ((rc = dalloc(h, &Q.boxpos, E * BD_MAXBOX))) return rc;
    if ((rc = dalloc(h, &Q.prev, E * BD_MAXBOX * 4))) return rc;
    if ((rc = dalloc(h, &Q.cum, E * 4))) return rc;
    if ((rc = dalloc(h, &Q.cnt, E * 4))) return rc;
    if ((rc = dalloc(h, &Q.wp, E * BD_MAXWP * 3))) return rc;
    if ((rc = dalloc(h, &Q.nwp, E))) return rc;
    if ((rc = dalloc(h, &Q.stepf, E * 8))) return rc;
    if ((rc = dalloc(h, &Q.unfin, E))) return rc;
    if ((rc = dalloc(h, &Q.rs_i, E * 16))) return rc;
    if ((rc = dalloc(h, &Q.rs_d, E * 132))) return rc;
    if ((rc = dalloc(h, &Q.straggler, (size_t)4))) return rc;
    if ((rc = dalloc(h, &Q.dist, E * NW))) return rc;
    if ((rc = dalloc(h, &Q.rmap, E * NW))) return rc;
    if ((rc = dalloc(h, &Q.cleared, E * BD_MAXBOX))) return rc;
    if ((rc = dalloc(h, &Q.m_box, E * BD_MAXBOX * 3))) return rc;
    d2 *d_goals;
    if ((rc = dalloc(h, &d_goals, 128))) return rc;
    if (cf.task == 1) HIPCHK(h, hipMemcpy(d_goals, cf.goal_points, sizeof(d2) * (size_t)cf.num_goal_points, hipMemcpyHostToDevice));
    Q.goals = d_goals;
    return BP_OK;
}
// Step 3: the dynamic-LDS size of each kernel family, and the limit of every kernel that may be launched with it
static int bd_lds_limits(bp_handle *h, int NW, int words)
{
    h->bd_lds = (size_t)words * 8 + (size_t)3 * BD_QCAP * 2 + 16 + (size_t)BD_PATHCAP * 2 * 2 + BD_PATHCAP + (size_t)BD_PATHCAP * 4 + (size_t)BD_MAXWP * 16 + 64;
    h->bd_obs_lds = (size_t)((NW + 15) & ~15);
    h->bd_rmap_lds = (((size_t)words + 3) & ~(size_t)3) * 4 + (size_t)3 * BD_QCAP * 2 + 16;
    if (h->bd_lds > 160 * 1024 || h->bd_obs_lds > 160 * 1024) return fail(h, BP_EINVAL, "map window too large for LDS");
    h->damp = h->P.damping_pow != 0.0;   // space.damping != 0: the generic instantiations (substep<BP_ENV_BOX, DAMP = true>)
    const struct { const void *kernel; size_t bytes; } limits[] = {
        {(const void *)k_bd_settle, h->lds_bytes},        {(const void *)k_bd_physics, h->lds_bytes},      {(const void *)k_bd_physics_resume, h->lds_bytes},
        {(const void *)k_bd_physics_damp, h->lds_bytes},  {(const void *)k_bd_slice, h->lds_bytes},        {(const void *)k_bd_slice_resume, h->lds_bytes},
        {(const void *)k_bd_settle_damp, h->lds_bytes},   {(const void *)k_bd_plan, h->bd_lds},            {(const void *)k_bd_plan_async, h->bd_lds},
        {(const void *)k_bd_finish, h->bd_lds},           {(const void *)k_ac_finish, h->bd_lds},          {(const void *)k_bd_observe, h->bd_obs_lds},
        {(const void *)k_bd_robot_map, h->bd_rmap_lds},
    };
    for (const auto &l : limits) HIPCHK(h, hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes));
    return BP_OK;
}
// Step 4: settle every trial once into its template slot, then the episode-start bookkeeping (box distances, robot map)
static int bd_settle_templates(bp_handle *h)
{
    const int T = h->num_trials;
    if (h->damp) hipLaunchKernelGGL(k_bd_settle_damp, dim3(T), dim3(64), h->lds_bytes, 0, h->P, h->D, (const unsigned char *)nullptr, (double *)nullptr, 1);
    else hipLaunchKernelGGL(k_bd_settle, dim3(T), dim3(64), h->lds_bytes, 0, h->P, h->D, (const unsigned char *)nullptr, (double *)nullptr, 1);
    HIPCHK(h, hipGetLastError());
    if (int rc = bd_finish(h, h->B, 0, StepOut{}, 1)) return rc;
    hipLaunchKernelGGL(k_bd_robot_map, dim3(T), dim3(BDR_THREADS), h->bd_rmap_lds, 0, h->P, h->D, h->B, h->Q, 1);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipDeviceSynchronize());
    return BP_OK;
}

int bp_bd_load(bp_handle *h, int32_t T, int32_t nbox, const double *starts, const double *boxes, int32_t ns, const double *sverts,
               const int32_t *scount, const double *spose, const double *srad, const int32_t *stype)
{
    if (!h || T <= 0 || nbox <= 0 || nbox > BD_MAXBOX || ns <= 0 || !starts || !boxes || !sverts || !scount || !spose || !srad || !stype) return BP_EINVAL;
    if (h->loaded) return fail(h, BP_ESTATE, "scenarios already loaded");
    if (h->P.env_kind != BP_ENV_BOX) return fail(h, BP_ESTATE, "handle was created for another environment");
    BP_DEVICE(h);
    bpgeom::BdScene sc;
    if (const char *e = bpgeom::bd_scene(h->bdcfg, T, nbox, starts, boxes, ns, sverts, scount, spose, srad, stype, sc)) return fail(h, BP_EINVAL, e);
    h->bd_maps = sc.maps;   // (bp_bd_get_maps) only now: a refused load leaves the handle as bp_bd_create made it
    h->bd_map_of_trial = sc.map_of_trial;
    int rc = upload_trials(h, sc.trials, false);
    if (rc) return rc;
    if (h->nbcap > 64) return fail(h, BP_EINVAL, "box-delivery supports at most 64 shape slots per env");
    BdParams &B = h->B;
    const bpgeom::BdMaps &M0 = sc.maps[0];
    B.H = M0.H; B.W = M0.W; B.SH = M0.SH; B.SW = M0.SW; B.si0 = M0.si0; B.sj0 = M0.sj0;
    B.nbox = nbox; B.nrecept = 1; B.out_r = M0.out_r;
    B.budget = 0; B.pass = 0; B.sel_want = -1; B.resume_sel = 0;
    // execute_robot_path skips whole periods once the robot's state recurs exactly (a robot that pushes against a wall until STEP_LIMIT); BP_BD_CYCLE=0: every sim step is run
    // (in the second pass of the two-pass step, whose envs are already beyond the first pass's budget: from the first sim step of the pass on; BP_BD_CYCLE=<n>: only
    //  once a path has run n sim steps)
    B.cycle_skip = getenv("BP_BD_CYCLE") ? std::max(0, atoi(getenv("BP_BD_CYCLE"))) : 1;
    // two-pass step: sim steps every env gets in pass 0 (the mean env needs ~750, the 99th percentile ~3 000; the reference's loops stop at 10 001); BP_BD_BUDGET=0: one pass
    h->bd_budget = getenv("BP_BD_BUDGET") ? atoi(getenv("BP_BD_BUDGET")) : 3000;
    const int NW = B.SH * B.SW, words = (NW + 31) / 32;
    if ((rc = bd_upload_maps(h, sc, NW, words))) return rc;
    if ((rc = bd_alloc_env_state(h, T, NW))) return rc;
    if ((rc = bd_lds_limits(h, NW, words))) return rc;
    if ((rc = bd_settle_templates(h))) return rc;
    if ((rc = state_setup(h))) return rc;
    h->loaded = true;
    return BP_OK;
}

int bp_bd_get_maps(bp_handle *h, int32_t trial, int32_t *dims, uint8_t *cspace, uint8_t *cspace_thin, uint16_t *edt, float *recept, uint8_t *small_free)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded || h->P.env_kind != BP_ENV_BOX) return fail(h, BP_ESTATE, "not a loaded box-delivery handle");
    if (trial < 0 || trial >= h->num_trials) return BP_EINVAL;
    const bpgeom::BdMaps &M = h->bd_maps[h->bd_map_of_trial[trial]];
    if (dims) { dims[0] = M.H; dims[1] = M.W; dims[2] = M.SH; dims[3] = M.SW; dims[4] = M.si0; dims[5] = M.sj0; }
    const int NW = M.SH * M.SW;
    for (int w = 0; w < NW; w++) {
        if (cspace) cspace[w] = (M.free_bits[w >> 5] >> (w & 31)) & 1u;
        if (cspace_thin) cspace_thin[w] = (M.thin_bits[w >> 5] >> (w & 31)) & 1u;
    }
    if (edt) memcpy(edt, M.edt.data(), sizeof(uint16_t) * NW * 2);
    if (recept) memcpy(recept, M.recept.data(), sizeof(float) * NW);
    if (small_free) memcpy(small_free, M.small_free.data(), NW);
    return BP_OK;
}

int bp_bd_get_state(bp_handle *h, uint8_t *alive, double *waypoints, int32_t *nwp)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded || h->P.env_kind != BP_ENV_BOX) return fail(h, BP_ESTATE, "not a loaded box-delivery handle");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    const size_t E = h->num_envs;
    if (alive) HIPCHK(h, hipMemcpy(alive, h->Q.alive, E * BD_MAXBOX, hipMemcpyDeviceToHost));
    if (waypoints) HIPCHK(h, hipMemcpy(waypoints, h->Q.wp, sizeof(double) * E * BD_MAXWP * 3, hipMemcpyDeviceToHost));
    if (nwp) HIPCHK(h, hipMemcpy(nwp, h->Q.nwp, sizeof(int) * E, hipMemcpyDeviceToHost));
    return BP_OK;
}

int32_t bp_sizeof_render_args(void) { return (int32_t)sizeof(bp_render_args); }
int32_t bp_sizeof_render_prim(void) { return (int32_t)sizeof(bp_render_prim); }

int bp_set_render_table(bp_handle *h, int32_t T, int32_t nslot, const int32_t *order, const uint32_t *rgb, int32_t nprim, const bp_render_prim *prims)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "render table before the scenarios are loaded");
    if (!order || !rgb || T != h->num_trials || nslot != h->nbcap)
        return fail(h, BP_EINVAL, "render table: order / rgb must be [num_trials][nb_cap] host arrays");
    if (nprim < 0 || nprim > BP_RENDER_MAX_PRIMS || (nprim > 0 && !prims)) return fail(h, BP_EINVAL, "render table: 0 <= nprim <= BP_RENDER_MAX_PRIMS");
    std::vector<bp_render_prim> pr;
    for (int layer = 0; layer < 2; layer++)
        for (int i = 0; i < nprim; i++) {
            const bp_render_prim &p = prims[i];
            if (p.layer != 0 && p.layer != 1) return fail(h, BP_EINVAL, "render primitive: layer must be 0 or 1");
            if (!((p.kind == 0 && p.nv >= 3 && p.nv <= BP_RENDER_PRIM_VERTS) || (p.kind == 1 && p.nv == 2)))
                return fail(h, BP_EINVAL, "render primitive: a polygon has 3..8 vertices, a capsule 2");
            if (p.layer == layer) pr.push_back(p);
        }
    const size_t n = (size_t)T * nslot;
    for (size_t i = 0; i < n; i++)
        if (order[i] < -1 || order[i] >= nslot) return fail(h, BP_EINVAL, "render table: slot index out of range");
    BP_DEVICE(h);
    int rc;
    if (!h->r_order) {
        if ((rc = dalloc(h, &h->r_order, n))) return rc;
        if ((rc = dalloc(h, &h->r_rgb, n))) return rc;
        if ((rc = dalloc(h, &h->r_prims, BP_RENDER_MAX_PRIMS))) return rc;
    }
    HIPCHK(h, hipMemcpy(h->r_order, order, sizeof(int) * n, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->r_rgb, rgb, sizeof(unsigned) * n, hipMemcpyHostToDevice));
    if (!pr.empty()) HIPCHK(h, hipMemcpy(h->r_prims, pr.data(), sizeof(bp_render_prim) * pr.size(), hipMemcpyHostToDevice));
    h->r_nunder = 0;
    for (const bp_render_prim &p : pr) h->r_nunder += p.layer == 0;
    h->r_nover = (int)pr.size() - h->r_nunder;
    h->r_table = true;
    return BP_OK;
}

int bp_render(bp_handle *h, const bp_render_args *args, const int32_t *env_ids, int32_t k, const double *paths, const int32_t *path_len,
              uint8_t *out, void *stream)
{
    if (!h) return BP_EINVAL;
    if (!args || !env_ids || !out) return fail(h, BP_EINVAL, "bp_render: null args, env_ids or out");
    if (k <= 0) return fail(h, BP_EINVAL, "bp_render: k must be positive");
    const bp_render_args &A = *args;
    if (!(A.scale > 0.0) || !std::isfinite(A.scale)) return fail(h, BP_EINVAL, "bp_render: scale must be positive");
    if (!std::isfinite(A.tx) || !std::isfinite(A.ty) || !std::isfinite(A.cx) || !std::isfinite(A.cy) || !std::isfinite(A.path_half_px))
        return fail(h, BP_EINVAL, "bp_render: transform must be finite");
    if (A.width <= 0 || A.height <= 0 || A.width > BP_RENDER_MAX_SIDE || A.height > BP_RENDER_MAX_SIDE ||
        (long long)A.width * A.height > BP_RENDER_MAX_PIXELS)
        return fail(h, BP_EINVAL, "bp_render: frame size outside 1..8192 per side / 2^24 pixels");
    if (A.max_path < 0 || A.max_path > BP_RENDER_MAX_PATH || ((paths == nullptr) != (path_len == nullptr)) || (paths && A.max_path == 0))
        return fail(h, BP_EINVAL, "bp_render: paths and path_len go together, with 1 <= max_path <= BP_RENDER_MAX_PATH");
    if (!h->loaded || !h->was_reset) return fail(h, BP_ESTATE, "not reset");
    if (!h->r_table) return fail(h, BP_ESTATE, "no render table (bp_set_render_table)");
    BP_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> ids(k);
    HIPCHK(h, hipMemcpyAsync(ids.data(), env_ids, sizeof(int) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int i = 0; i < k; i++)
        if (ids[i] < 0 || ids[i] >= h->num_envs) return fail(h, BP_EINVAL, "bp_render: env id " + std::to_string(ids[i]) + " outside the batch");
    RenderK K;
    K.wv = h->D.wv; K.sc_nv = h->D.sc_nv; K.sc_prop = h->D.sc_prop; K.e_trial = h->D.e_trial; K.e_nb = h->D.e_nb;
    const bool box = h->P.env_kind == BP_ENV_BOX;
    K.alive = box ? h->Q.alive : nullptr; K.first_box = box ? h->B.first_box : 0; K.nbox = box ? h->B.nbox : 0;
    K.nbcap = h->nbcap; K.num_envs = h->num_envs; K.num_trials = h->num_trials;
    K.order = h->r_order; K.rgb = h->r_rgb; K.prims = h->r_prims; K.nslot = h->nbcap; K.nunder = h->r_nunder; K.nover = h->r_nover;
    K.env_ids = env_ids; K.paths = paths; K.path_len = path_len; K.max_path = paths ? A.max_path : 0;
    K.width = A.width; K.height = A.height;
    K.tiles_x = (A.width + RENDER_TW - 1) / RENDER_TW;
    K.tiles = K.tiles_x * ((A.height + RENDER_TH - 1) / RENDER_TH);
    K.scale = A.scale; K.tx = A.tx; K.ty = A.ty; K.cx = A.cx; K.cy = A.cy; K.path_half = A.path_half_px;
    K.background = A.background & 0xFFFFFFu; K.out = out;
    const int chunk = std::max(1, (1 << 22) / K.tiles);    // frames per launch: at most 2^22 workgroups
    for (int f0 = 0; f0 < k; f0 += chunk) {
        K.frame0 = f0;
        const int nf = std::min(chunk, k - f0);
        hipLaunchKernelGGL(k_render, dim3((unsigned)(nf * K.tiles)), dim3(RENDER_THREADS), 0, st, K);
        HIPCHK(h, hipGetLastError());
    }
    return BP_OK;
}

// ---- state records (bp_state.hpp) --------------------------------------------------------------------------------------------------------------
int64_t bp_state_bytes(const bp_handle *h)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded || !h->st_table) return BP_ESTATE;
    return (int64_t)h->st_layout.bytes;
}
uint64_t bp_state_layout_id(const bp_handle *h) { return (h && h->loaded && h->st_table) ? h->st_layout_id : 0; }

int bp_state_layout_query(int32_t env_kind, int32_t task, int32_t nbcap, int32_t map_cells, int32_t max_segments, int64_t *offsets_host,
                          int64_t *bytes_host, int32_t *widths_host, int64_t *total_bytes, uint64_t *structure_id)
{
    if (env_kind < BP_ENV_SHIP_ICE || env_kind > BP_ENV_BOX || nbcap <= 0 || (nbcap & 7) || map_cells < 0 || max_segments < 0) return BP_EINVAL;
    const bool box = env_kind == BP_ENV_BOX;
    if ((box && map_cells == 0) || (!box && (map_cells != 0 || task != 0)) || task < 0 || task > 1) return BP_EINVAL;
    DevPtrs D; BdPtrs Q;
    memset(&D, 0, sizeof(D)); memset(&Q, 0, sizeof(Q));
    const BpStateLayout L = bp_state_layout(D, Q, nbcap, box, map_cells);
    for (int i = 0; i < L.nseg && i < max_segments; i++) {
        if (offsets_host) offsets_host[i] = (int64_t)L.seg[i].off;
        if (bytes_host) bytes_host[i] = (int64_t)L.seg[i].span;
        if (widths_host) widths_host[i] = (int32_t)L.seg[i].width;
    }
    if (total_bytes) *total_bytes = (int64_t)L.bytes;
    if (structure_id) *structure_id = bp_state_structure_id(L, env_kind, task, nbcap, map_cells);
    return L.nseg;
}

// ids on the host (one synchronisation of the stream, as bp_render does for its ids): every id inside [0, E); no id of `dst` twice; no id of `dst` among `src`
static int state_check_ids(bp_handle *h, const char *what, const int32_t *dst, const int32_t *src, int k, hipStream_t st, const uint8_t *records)
{
    std::vector<int> d(k), s(src ? k : 0);
    std::vector<BpStateHeader> hdr(records ? k : 0);
    HIPCHK(h, hipMemcpyAsync(d.data(), dst, sizeof(int) * k, hipMemcpyDeviceToHost, st));
    if (src) HIPCHK(h, hipMemcpyAsync(s.data(), src, sizeof(int) * k, hipMemcpyDeviceToHost, st));
    if (records) HIPCHK(h, hipMemcpy2DAsync(hdr.data(), sizeof(BpStateHeader), records, (size_t)h->st_layout.bytes, sizeof(BpStateHeader), (size_t)k, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    std::vector<unsigned char> seen(h->num_envs, 0);
    for (int i = 0; i < k; i++) {
        if (d[i] < 0 || d[i] >= h->num_envs) return fail(h, BP_EINVAL, std::string(what) + ": env id " + std::to_string(d[i]) + " outside the batch");
        if (src || records) {   // destinations: none twice
            if (seen[d[i]]) return fail(h, BP_EINVAL, std::string(what) + ": destination env " + std::to_string(d[i]) + " is named twice");
            seen[d[i]] = 1;
        }
    }
    for (int i = 0; i < (src ? k : 0); i++) {
        if (s[i] < 0 || s[i] >= h->num_envs) return fail(h, BP_EINVAL, std::string(what) + ": env id " + std::to_string(s[i]) + " outside the batch");
        if (seen[s[i]]) return fail(h, BP_EINVAL, std::string(what) + ": env " + std::to_string(s[i]) + " is both a source and a destination");
    }
    for (int i = 0; i < (records ? k : 0); i++)
        if (hdr[i].magic != BP_STATE_MAGIC || hdr[i].bytes != h->st_layout.bytes || hdr[i].layout_id != h->st_layout_id)
            return fail(h, BP_EINVAL, std::string(what) + ": record " + std::to_string(i) + (hdr[i].magic != BP_STATE_MAGIC ? " is not a state record" :
                        " was saved by a handle with another configuration, trials or capacities (layout id)"));
    return BP_OK;
}

static int state_launch(const int MODE, bp_handle *h, const int *ids_a, const int *ids_b, unsigned char *records, int k, hipStream_t st)
{
    StateArgs A;
    A.table = h->st_table; A.nseg = h->st_layout.nseg; A.nslots = (unsigned)(h->st_layout.bytes >> 4);
    A.ids_a = ids_a; A.ids_b = ids_b; A.records = records;
    A.hdr.magic = BP_STATE_MAGIC; A.hdr.bytes = h->st_layout.bytes; A.hdr.layout_id = h->st_layout_id; A.hdr.reserved = 0;
    // four slots per thread in flight when that still leaves a workgroup for every wave slot or so of the device; one slot per thread for small k
    const unsigned tiles4 = (A.nslots + 4 * BP_STATE_THREADS - 1) / (4 * BP_STATE_THREADS);
    const bool wide = (unsigned long long)k * tiles4 >= 2048ull;
    A.tiles = wide ? tiles4 : (A.nslots + BP_STATE_THREADS - 1) / BP_STATE_THREADS;
    const int chunk = std::max(1, (int)((1u << 30) / A.tiles));   // records per launch
    for (int r0 = 0; r0 < k; r0 += chunk) {
        A.rec0 = r0;
        const dim3 grid((unsigned)std::min(chunk, k - r0) * A.tiles), block(BP_STATE_THREADS);
        if (MODE == STATE_PACK) { if (wide) hipLaunchKernelGGL(k_state_pack<4>, grid, block, 0, st, A); else hipLaunchKernelGGL(k_state_pack<1>, grid, block, 0, st, A); }
        else if (MODE == STATE_UNPACK) { if (wide) hipLaunchKernelGGL(k_state_unpack<4>, grid, block, 0, st, A); else hipLaunchKernelGGL(k_state_unpack<1>, grid, block, 0, st, A); }
        else { if (wide) hipLaunchKernelGGL(k_state_clone<4>, grid, block, 0, st, A); else hipLaunchKernelGGL(k_state_clone<1>, grid, block, 0, st, A); }
        HIPCHK(h, hipGetLastError());
    }
    return BP_OK;
}

static int state_ready(bp_handle *h, const char *what)
{
    if (!h->loaded || !h->was_reset || !h->st_table) return fail(h, BP_ESTATE, std::string(what) + " before the first bp_reset");
    return BP_OK;
}

int bp_save_state(bp_handle *h, const int32_t *env_ids, int32_t k, uint8_t *records, void *stream)
{
    if (!h) return BP_EINVAL;
    if (int rc = state_ready(h, "bp_save_state")) return rc;
    if (h->async_open) return fail(h, BP_ESTATE, "bp_save_state while an asynchronous slice is open: state records do not carry the loop state of a busy env");
    if (!env_ids || !records || k <= 0 || ((uintptr_t)records & 15u)) return fail(h, BP_EINVAL, "bp_save_state: null env_ids / records, k <= 0 or records not 16-byte aligned");
    BP_DEVICE(h);
    if (int rc = state_check_ids(h, "bp_save_state", env_ids, nullptr, k, (hipStream_t)stream, nullptr)) return rc;
    return state_launch(STATE_PACK, h, env_ids, nullptr, records, k, (hipStream_t)stream);
}

int bp_load_state(bp_handle *h, const int32_t *env_ids, int32_t k, const uint8_t *records, int32_t flags, void *stream)
{
    if (!h) return BP_EINVAL;
    if (int rc = state_ready(h, "bp_load_state")) return rc;
    if (h->async_open) return fail(h, BP_ESTATE, "bp_load_state while an asynchronous slice is open: state records do not carry the loop state of a busy env");
    if (!env_ids || !records || k <= 0 || ((uintptr_t)records & 15u)) return fail(h, BP_EINVAL, "bp_load_state: null env_ids / records, k <= 0 or records not 16-byte aligned");
    BP_DEVICE(h);
    if (!(flags & BP_STATE_TRUSTED))
        if (int rc = state_check_ids(h, "bp_load_state", env_ids, nullptr, k, (hipStream_t)stream, records)) return rc;
    return state_launch(STATE_UNPACK, h, env_ids, nullptr, const_cast<uint8_t *>(records), k, (hipStream_t)stream);
}

int bp_clone_state(bp_handle *h, const int32_t *src_ids, const int32_t *dst_ids, int32_t k, int32_t flags, void *stream)
{
    if (!h) return BP_EINVAL;
    if (int rc = state_ready(h, "bp_clone_state")) return rc;
    if (h->async_open) return fail(h, BP_ESTATE, "bp_clone_state while an asynchronous slice is open: state records do not carry the loop state of a busy env");
    if (!src_ids || !dst_ids || k <= 0) return fail(h, BP_EINVAL, "bp_clone_state: null ids or k <= 0");
    BP_DEVICE(h);
    if (!(flags & BP_STATE_TRUSTED))
        if (int rc = state_check_ids(h, "bp_clone_state", dst_ids, src_ids, k, (hipStream_t)stream, nullptr)) return rc;
    return state_launch(STATE_CLONE, h, src_ids, dst_ids, nullptr, k, (hipStream_t)stream);
}

int bp_get_num_bodies(bp_handle *h, int32_t *out_host)
{
    if (!h || !out_host) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out_host, h->D.e_nb, sizeof(int) * h->num_envs, hipMemcpyDeviceToHost));
    return BP_OK;
}

int bp_check_errors(bp_handle *h, int32_t *out_host)
{
    if (!h) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<int> e(h->num_envs);
    HIPCHK(h, hipMemcpy(e.data(), h->D.e_err, sizeof(int) * h->num_envs, hipMemcpyDeviceToHost));
    int any = 0;
    for (int v : e) any |= v;
    if (out_host) memcpy(out_host, e.data(), sizeof(int) * h->num_envs);
    if (any) return fail(h, BP_ECAPACITY, "in-kernel capacity overflow, bits=" + std::to_string(any));
    return BP_OK;
}

int bp_get_step_cycles(bp_handle *h, uint32_t *out_host)
{
    if (!h || !out_host) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out_host, h->D.e_cost, sizeof(unsigned) * h->num_envs, hipMemcpyDeviceToHost));
    return BP_OK;
}

int32_t bp_sched_chunk(bp_handle *h) { return h ? h->sched_chunk : 0; }
int32_t bp_sched_resident(bp_handle *h)
{
    if (!h || h->sched_chunk <= 0 || (h->resident_auto && h->device_shared)) return 0;
    return h->P.pair_mode == 2 ? h->pair_resident : h->sched_persist;
}
int32_t bp_device_shared(bp_handle *h) { return (h && h->resident_auto && h->device_shared) ? 1 : 0; }
int32_t bp_bd_budget(bp_handle *h) { return h ? h->bd_budget : 0; }
int bp_launch_policy_query(int32_t num_envs, int32_t num_compute_units, int32_t can_pair, int32_t is_maze, int32_t *out8_host)
{
    if (!out8_host || num_envs <= 0 || num_compute_units <= 0) return BP_EINVAL;
    const BpLaunchPolicy p = bp_launch_policy(num_envs, num_compute_units, can_pair != 0, is_maze != 0);
    out8_host[0] = p.wave_slots; out8_host[1] = p.pair_mode; out8_host[2] = p.tight; out8_host[3] = p.pair_solo; out8_host[4] = p.chunk;
    out8_host[5] = p.pp_max_act; out8_host[6] = p.pp_max_work; out8_host[7] = p.pp_rate;
    return BP_OK;
}

int bp_get_clock_stamps(bp_handle *h, uint64_t *out16_host)
{
    uint64_t *out2_host = out16_host;
    if (!h || !out2_host) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out2_host, h->D.clk, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return BP_OK;
}

int32_t bp_pair_mode(bp_handle *h) { return h ? h->pair_mode : 0; }

int bp_bd_get_stragglers(bp_handle *h, uint32_t *out2_host)
{
    if (!h || !out2_host) return BP_EINVAL;
    if (!h->loaded || h->P.env_kind != BP_ENV_BOX || h->Q.straggler == nullptr) return fail(h, BP_ESTATE, "not a loaded box-delivery / area-clearing handle");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out2_host, h->Q.straggler, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BP_OK;
}
int bp_bd_get_cycle_skips(bp_handle *h, uint32_t *out2_host)
{
    if (!h || !out2_host) return BP_EINVAL;
    if (!h->loaded || h->P.env_kind != BP_ENV_BOX || h->Q.straggler == nullptr) return fail(h, BP_ESTATE, "not a loaded box-delivery / area-clearing handle");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out2_host, h->Q.straggler + 2, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BP_OK;
}

int bp_get_pair_stats(bp_handle *h, int32_t *out16_host)
{
    if (!h || !out16_host) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    const DevParams &P = h->P;
    const int32_t par[8] = {h->pair_mode, P.pair_solo, P.pp_max_keys, P.pp_max_slots, P.pp_max_mv, P.pp_max_act, P.pp_max_work, P.pp_rate};
    memcpy(out16_host, par, sizeof(par));
    memset(out16_host + 8, 0, 8 * sizeof(int32_t));
    if (h->D.sq_pairstat != nullptr) {
        HIPCHK(h, hipDeviceSynchronize());
        HIPCHK(h, hipMemcpy(out16_host + 8, h->D.sq_pairstat, 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return BP_OK;
}

int bp_sched_warnings(bp_handle *h, int32_t *out2_host)
{
    if (!h || !out2_host) return BP_EINVAL;
    out2_host[0] = out2_host[1] = 0;
    if (h->sched_chunk <= 0 || !h->D.sq_warn) return BP_OK;
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out2_host, h->D.sq_warn, 2 * sizeof(int), hipMemcpyDeviceToHost));
    return BP_OK;
}

int bp_set_step_cost_hint(bp_handle *h, const uint32_t *host_costs)
{
    if (!h || !host_costs) return BP_EINVAL;
    if (!h->loaded) return fail(h, BP_ESTATE, "not loaded");
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(h->D.e_cost, host_costs, sizeof(unsigned) * h->num_envs, hipMemcpyHostToDevice));
    return BP_OK;
}

int bp_enable_timing(bp_handle *h, int32_t on)
{
    if (!h) return BP_EINVAL;
    h->timing = on != 0;
    h->ev_used = 0;
    if (on && h->loaded && h->P.env_kind != BP_ENV_BOX) {   // per-launch cost statistics ride along (bp_get_cost_stats)
        BP_DEVICE(h);
        if (!h->cost_ring) { int rc = dalloc(h, &h->cost_ring, (size_t)BP_COST_RING * 2); if (rc) return rc; }
        h->cost_n = 0;
    }
    return BP_OK;
}

int bp_get_cost_stats(bp_handle *h, uint64_t *out_host, int32_t max_launches, int32_t *launches)
{
    if (!h || !launches || (max_launches > 0 && !out_host)) return BP_EINVAL;
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    const int n = std::min(h->cost_n, std::max(0, (int)max_launches));
    if (n > 0) HIPCHK(h, hipMemcpy(out_host, h->cost_ring, (size_t)n * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *launches = n;
    return BP_OK;
}

int bp_kernel_time_ms(bp_handle *h, double *physics_ms, double *raster_ms, int32_t *launches)
{
    if (!h) return BP_EINVAL;
    BP_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    double p = 0, r = 0;
    const int n = (int)(h->ev_used / 3);
    for (int k = 0; k < n; k++) {
        float a = 0, b = 0;
        HIPCHK(h, hipEventElapsedTime(&a, h->ev[3 * k], h->ev[3 * k + 1]));
        HIPCHK(h, hipEventElapsedTime(&b, h->ev[3 * k + 1], h->ev[3 * k + 2]));
        p += a; r += b;
    }
    if (physics_ms) *physics_ms = n ? p / n : 0.0;
    if (raster_ms) *raster_ms = n ? r / n : 0.0;
    if (launches) *launches = n;
    h->ev_used = 0;
    return BP_OK;
}

// reset() normally copies the per-trial settled template (a pure function of the trial); on != 0 makes it re-run the
// 1000 settle sub-steps in place like the reference does (same result; used by the tests to prove that).
int bp_set_resettle(bp_handle *h, int32_t on)
{
    if (!h) return BP_EINVAL;
    h->resettle = (on != 0) || (h->P.random_start != 0); // per-episode start poses always settle in place
    return BP_OK;
}

// ---- replay buffer on the ready queue (bp_replay.hpp): handle-free, the caller owns the memory ----
int32_t bp_sizeof_replay_desc(void) { return (int32_t)sizeof(bp_replay_desc); }
int32_t bp_sizeof_replay_batch(void) { return (int32_t)sizeof(bp_replay_batch); }
int64_t bp_replay_index(uint64_t seed, int64_t draw, int32_t b, int64_t n)
{
    if (n < 1 || n > 0x7FFFFFFFll || b < 0) return -1;
    return bp_replay_pick(seed, draw, b, n);
}
static int replay_buf(const bp_replay_desc *d, ReplayBuf *r)
{
    if (!d || !d->state || !d->next_state || !d->action || !d->reward || !d->ministeps || !d->nonfinal || !d->env || !d->pend_obs || !d->pend_action ||
        !d->pend_flags || !d->hdr || !d->row_slot || !d->win)
        return BP_EINVAL;
    if (d->capacity < 1 || d->num_envs < 1 || d->action_dim != 1 || d->max_rows < 1 || d->device < 0) return BP_EINVAL;
    if (d->row_bytes < 16 || d->row_bytes % 16 != 0 || d->row_bytes / 16 > 0x7FFFFFFFll) return BP_EINVAL;
    if ((((uintptr_t)d->state | (uintptr_t)d->next_state | (uintptr_t)d->pend_obs) & 15u) != 0) return BP_EINVAL;
    r->C = d->capacity; r->E = d->num_envs; r->row16 = (int)(d->row_bytes / 16);
    r->state = (uint4 *)d->state; r->next_state = (uint4 *)d->next_state; r->action = d->action; r->reward = d->reward; r->ministeps = d->ministeps;
    r->nonfinal = d->nonfinal; r->env = d->env; r->pend_obs = (uint4 *)d->pend_obs; r->pend_action = d->pend_action; r->pend_flags = d->pend_flags;
    r->hdr = (long long *)d->hdr; r->row_slot = d->row_slot; r->win = d->win;
    return BP_OK;
}
static int replay_pieces(const ReplayBuf &r) { return (r.row16 + RPL_COPY_THREADS - 1) / RPL_COPY_THREADS; }
int bp_replay_observe(const bp_replay_desc *d, const int32_t *ids, const uint8_t *obs, const double *reward, const uint8_t *terminated,
                      const uint8_t *truncated, const double *info, const int32_t *slices, int32_t M, int32_t ministeps_col, void *stream)
{
    ReplayBuf r;
    if (replay_buf(d, &r) != BP_OK || !ids || !obs || !reward || !terminated || !truncated || !info || !slices) return BP_EINVAL;
    if (M < 1 || M > d->max_rows || ministeps_col < 0 || ministeps_col >= BP_INFO_COUNT || (((uintptr_t)obs) & 15u) != 0) return BP_EINVAL;
    if (replay_pieces(r) > 65535) return BP_EINVAL;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_replay_plan, dim3(1), dim3(RPL_THREADS), 0, st, r, (const int *)ids, reward, (const unsigned char *)terminated, info,
                       (const int *)slices, M, BP_INFO_COUNT, ministeps_col);
    hipLaunchKernelGGL(k_replay_copy, dim3(M, replay_pieces(r)), dim3(RPL_COPY_THREADS), 0, st, r, (const int *)ids, (const uint4 *)obs);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}
int bp_replay_record(const bp_replay_desc *d, const double *actions, const int32_t *ids, const uint8_t *reset, int32_t M, void *stream)
{
    ReplayBuf r;
    if (replay_buf(d, &r) != BP_OK || !actions || !ids || M < 1) return BP_EINVAL;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipLaunchKernelGGL(k_replay_record, dim3(1), dim3(RPL_THREADS), 0, (hipStream_t)stream, r, actions, (const int *)ids, (const unsigned char *)reset, M);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}
int bp_replay_sample(const bp_replay_desc *d, int32_t B, uint64_t seed, const bp_replay_batch *out, void *stream)
{
    ReplayBuf r;
    if (replay_buf(d, &r) != BP_OK || !out || B < 1) return BP_EINVAL;
    if (!out->state || !out->next_state || !out->action || !out->reward || !out->ministeps || !out->nonfinal || !out->slot || !out->valid) return BP_EINVAL;
    if ((((uintptr_t)out->state | (uintptr_t)out->next_state) & 15u) != 0 || replay_pieces(r) > 65535) return BP_EINVAL;
    ReplayBatch o;
    o.state = out->state; o.next_state = out->next_state; o.action = (long long *)out->action; o.reward = out->reward; o.ministeps = out->ministeps;
    o.nonfinal = out->nonfinal; o.slot = out->slot; o.valid = out->valid;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_replay_pick, dim3(1), dim3(RPL_THREADS), 0, st, r, o, B, (unsigned long long)seed);
    hipLaunchKernelGGL(k_replay_gather, dim3(B, replay_pieces(r)), dim3(RPL_COPY_THREADS), 0, st, r, o);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}

// ---- on-policy rollout buffer with GAE (bp_rollout.hpp): handle-free, the caller owns the memory ----
int32_t bp_sizeof_rollout_desc(void) { return (int32_t)sizeof(bp_rollout_desc); }
int32_t bp_sizeof_rollout_batch(void) { return (int32_t)sizeof(bp_rollout_batch); }
int64_t bp_rollout_index(uint64_t seed, int64_t epoch, int64_t i, int64_t n)
{
    if (n < 1 || n > 0x7FFFFFFFll || i < 0 || i >= n) return -1;
    return bp_rollout_perm(seed, epoch, i, n);
}
static int rollout_strips(const RolloutBuf &r)
{
    const int pieces = (r.row16 + RPL_COPY_THREADS - 1) / RPL_COPY_THREADS;
    return pieces < RLO_ROW_STRIPS ? pieces : RLO_ROW_STRIPS;
}
static int rollout_buf(const bp_rollout_desc *d, RolloutBuf *r)
{
    if (!d || !d->obs || !d->action || !d->reward || !d->value || !d->logp || !d->advantage || !d->ret || !d->episode_start || !d->last_done || !d->hdr)
        return BP_EINVAL;
    if (d->n_steps < 1 || d->num_envs < 1 || d->action_dim < 1 || d->device < 0) return BP_EINVAL;
    if ((int64_t)d->n_steps * d->num_envs > 0x7FFFFFFFll || (int64_t)d->num_envs * d->action_dim > 0x7FFFFFFFll) return BP_EINVAL;
    if (d->row_bytes < 16 || d->row_bytes % 16 != 0 || d->row_bytes / 16 > 0x7FFFFFFFll) return BP_EINVAL;
    if ((((uintptr_t)d->obs) & 15u) != 0) return BP_EINVAL;
    r->T = d->n_steps; r->E = d->num_envs; r->A = d->action_dim; r->row16 = (int)(d->row_bytes / 16);
    r->obs = (uint4 *)d->obs; r->action = d->action; r->reward = d->reward; r->value = d->value; r->logp = d->logp; r->advantage = d->advantage;
    r->ret = d->ret; r->episode_start = d->episode_start; r->last_done = d->last_done; r->hdr = (long long *)d->hdr;
    return BP_OK;
}
int bp_rollout_begin(const bp_rollout_desc *d, int32_t t, const uint8_t *obs, const float *action, const float *value, const float *logp, void *stream)
{
    RolloutBuf r;
    if (rollout_buf(d, &r) != BP_OK || !obs || !action || !value || !logp || t < 0 || t >= d->n_steps || (((uintptr_t)obs) & 15u) != 0) return BP_EINVAL;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    int64_t n = (int64_t)r.E * r.row16;               // pieces of the batch; E * A and E threads ride along
    if ((int64_t)r.E * r.A > n) n = (int64_t)r.E * r.A;
    int64_t blocks = (n + RPL_COPY_THREADS - 1) / RPL_COPY_THREADS;
    if (blocks > RLO_COPY_BLOCKS) blocks = RLO_COPY_BLOCKS;
    hipLaunchKernelGGL(k_rollout_begin, dim3((unsigned)blocks), dim3(RPL_COPY_THREADS), 0, (hipStream_t)stream, r, (int)t, (const uint4 *)obs, action, value, logp);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}
int bp_rollout_pick_rows(const bp_rollout_desc *d, const uint8_t *mask, const uint8_t *src, int32_t K, int32_t *out_ids, float *out_rows, void *stream)
{
    RolloutBuf r;
    if (rollout_buf(d, &r) != BP_OK || !mask || !src || !out_ids || !out_rows || K < 1) return BP_EINVAL;
    if (((((uintptr_t)src) | ((uintptr_t)out_rows)) & 15u) != 0) return BP_EINVAL;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rollout_pick, dim3(1), dim3(RPL_THREADS), 0, st, r, (const unsigned char *)mask, (int)K, (int *)out_ids);
    hipLaunchKernelGGL(k_rollout_rows, dim3(K, rollout_strips(r)), dim3(RPL_COPY_THREADS), 0, st, (const uint4 *)src, (const int *)out_ids,
                       (const unsigned char *)nullptr, (long long)r.E, r.row16, out_rows);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}
int bp_rollout_end(const bp_rollout_desc *d, int32_t t, const double *reward, const uint8_t *done, const int32_t *boot_ids, const float *boot_values,
                   int32_t K, double gamma, void *stream)
{
    RolloutBuf r;
    if (rollout_buf(d, &r) != BP_OK || !reward || !done || t < 0 || t >= d->n_steps) return BP_EINVAL;
    if (boot_ids && (!boot_values || K < 1)) return BP_EINVAL;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipLaunchKernelGGL(k_rollout_end, dim3(1), dim3(RPL_THREADS), 0, (hipStream_t)stream, r, (int)t, reward, (const unsigned char *)done,
                       (const int *)boot_ids, boot_values, boot_ids ? (int)K : 0, (float)gamma);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}
int bp_rollout_finish(const bp_rollout_desc *d, const float *last_values, double gamma, double gl, void *stream)
{
    RolloutBuf r;
    if (rollout_buf(d, &r) != BP_OK || !last_values) return BP_EINVAL;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipLaunchKernelGGL(k_rollout_gae, dim3((r.E + RLO_GAE_THREADS - 1) / RLO_GAE_THREADS), dim3(RLO_GAE_THREADS), 0, (hipStream_t)stream, r, last_values,
                       (float)gamma, (float)gl);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}
int bp_rollout_minibatch(const bp_rollout_desc *d, uint64_t seed, int64_t epoch, int32_t j, int32_t B, const bp_rollout_batch *out, void *stream)
{
    RolloutBuf r;
    if (rollout_buf(d, &r) != BP_OK || !out || B < 1 || j < 0 || (int64_t)j * B >= (int64_t)d->n_steps * d->num_envs) return BP_EINVAL;
    if (!out->obs || !out->action || !out->value || !out->logp || !out->advantage || !out->ret || !out->index || !out->valid) return BP_EINVAL;
    if ((((uintptr_t)out->obs) & 15u) != 0) return BP_EINVAL;
    RolloutBatch o;
    o.obs = out->obs; o.action = out->action; o.value = out->value; o.logp = out->logp; o.advantage = out->advantage; o.ret = out->ret;
    o.index = out->index; o.valid = out->valid;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rollout_index, dim3((B + RPL_COPY_THREADS - 1) / RPL_COPY_THREADS), dim3(RPL_COPY_THREADS), 0, st, r, o, (unsigned long long)seed,
                       (long long)epoch, (long long)j * B, (int)B);
    hipLaunchKernelGGL(k_rollout_rows, dim3(B, rollout_strips(r)), dim3(RPL_COPY_THREADS), 0, st, (const uint4 *)r.obs, (const int *)o.index,
                       (const unsigned char *)o.valid, (long long)r.T * r.E, r.row16, o.obs);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}

// ---- transition buffer for lock-step envs (bp_transitions.hpp): handle-free, the caller owns the memory ----
int32_t bp_sizeof_transitions_desc(void) { return (int32_t)sizeof(bp_transitions_desc); }
int32_t bp_sizeof_transitions_batch(void) { return (int32_t)sizeof(bp_transitions_batch); }
static int trans_strips(const TransBuf &r, int64_t rows)   // workgroups per row: RLO_ROW_STRIPS, more while rows * strips stays below TRN_MIN_GROUPS
{
    const int64_t pieces = ((int64_t)r.row16 + RPL_COPY_THREADS - 1) / RPL_COPY_THREADS;
    int64_t want = (TRN_MIN_GROUPS + rows - 1) / rows;
    if (want < RLO_ROW_STRIPS) want = RLO_ROW_STRIPS;
    return (int)(pieces < want ? pieces : want);
}
static int trans_buf(const bp_transitions_desc *d, TransBuf *r)
{
    if (!d || !d->obs || !d->next_obs || !d->action || !d->reward || !d->done || !d->timeout || !d->hdr) return BP_EINVAL;
    if (d->steps < 1 || d->num_envs < 1 || d->action_dim < 1 || d->device < 0) return BP_EINVAL;
    if ((int64_t)d->steps * d->num_envs > 0x7FFFFFFFll || (int64_t)d->num_envs * d->action_dim > 0x7FFFFFFFll) return BP_EINVAL;
    if (d->row_bytes < 16 || d->row_bytes % 16 != 0 || d->row_bytes / 16 > 0x7FFFFFFFll) return BP_EINVAL;
    if (((((uintptr_t)d->obs) | ((uintptr_t)d->next_obs)) & 15u) != 0) return BP_EINVAL;
    r->T = d->steps; r->E = d->num_envs; r->A = d->action_dim; r->row16 = (int)(d->row_bytes / 16);
    r->obs = (uint4 *)d->obs; r->next_obs = (uint4 *)d->next_obs; r->action = d->action; r->reward = d->reward; r->done = d->done;
    r->timeout = d->timeout; r->hdr = (long long *)d->hdr;
    return BP_OK;
}
int bp_transitions_add(const bp_transitions_desc *d, const uint8_t *obs, const uint8_t *next_obs, const uint8_t *terminal_obs, const float *action,
                       const double *reward, const uint8_t *done, const uint8_t *truncated, void *stream)
{
    TransBuf r;
    if (trans_buf(d, &r) != BP_OK || !obs || !next_obs || !terminal_obs || !action || !reward || !done || !truncated) return BP_EINVAL;
    if (((((uintptr_t)obs) | ((uintptr_t)next_obs) | ((uintptr_t)terminal_obs)) & 15u) != 0) return BP_EINVAL;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_trans_rows, dim3(r.E, trans_strips(r, r.E)), dim3(RPL_COPY_THREADS), 0, st, r, (const uint4 *)obs, (const uint4 *)next_obs,
                       (const uint4 *)terminal_obs, (const unsigned char *)done);
    hipLaunchKernelGGL(k_trans_scalars, dim3(1), dim3(RPL_THREADS), 0, st, r, action, reward, (const unsigned char *)done, (const unsigned char *)truncated);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}
int bp_transitions_sample(const bp_transitions_desc *d, uint64_t seed, int32_t B, const bp_transitions_batch *out, void *stream)
{
    TransBuf r;
    if (trans_buf(d, &r) != BP_OK || !out || B < 1) return BP_EINVAL;
    if (!out->obs || !out->next_obs || !out->action || !out->reward || !out->done || !out->slot || !out->valid) return BP_EINVAL;
    if (((((uintptr_t)out->obs) | ((uintptr_t)out->next_obs)) & 15u) != 0 || (int64_t)B * d->action_dim > 0x7FFFFFFFll) return BP_EINVAL;
    TransBatch o;
    o.obs = out->obs; o.next_obs = out->next_obs; o.action = out->action; o.reward = out->reward; o.done = out->done; o.slot = out->slot;
    o.valid = out->valid;
    DevGuard dg(d->device);
    if (!dg.ok) return BP_EHIP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_trans_pick, dim3(1), dim3(RPL_THREADS), 0, st, r, o, (int)B, (unsigned long long)seed);
    hipLaunchKernelGGL(k_trans_gather, dim3(B, trans_strips(r, B), 2), dim3(RPL_COPY_THREADS), 0, st, r, o);
    return hipGetLastError() == hipSuccess ? BP_OK : BP_EHIP;
}

// debug hook of the diagnostic twin (-DBP_DEBUG_PATHS): trace (x, y, angle) of every body of one env after each sub-step of the next
// launches into a device buffer [substeps][nb_cap][3]; pass NULL to disable.
int bp_debug_trace(bp_handle *h, double *dev_buf, int32_t env)
{
    if (!h) return BP_EINVAL;
#ifndef BP_DEBUG_PATHS
    // the product kernels do not test the trace pointer every sub-step; the diagnostic twin does (benchpush_amd/build.py: build_debug_paths)
    if (dev_buf) return fail(h, BP_ESTATE, "bp_debug_trace needs the -DBP_DEBUG_PATHS build (BP_PROF=1 BP_PROF_LIB=.../libbenchpush_hip_dbgpaths.so)");
#endif
    h->D.dbg = dev_buf;
    h->D.dbg_env = env;
    return BP_OK;
}

// diagnostic builds (-DBP_PROF): per-env phase cycle counters, device buffer [E][24] u64 or NULL
int bp_debug_prof(bp_handle *h, unsigned long long *dev_buf)
{
    if (!h) return BP_EINVAL;
    h->D.prof = dev_buf;
    return BP_OK;
}

} // extern "C"
