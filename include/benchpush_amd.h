/*
 * benchpush_amd.h -- C ABI of the MI355X-native batched ship-ice environment (libbenchpush_hip.so).
 *
 * The reference (IvanIZ/BenchPush) is pure Python and has no FFI for this path: the hot path is
 * ShipIceEnv.step()/reset() calling pymunk.Space.step 400x per step plus pure-python rasters
 * (benchpush/environments/ship_ice_nav/ship_ice_env.py:223-355,378-409).  This ABI is what a ctypes
 * binding inside the reference's ShipIceEnv would bind instead; each entry point
 * cites the reference code it replaces.
 *
 * Conventions: every function returns 0 on success or a negative BP_E* code, never throws; the caller
 * owns all buffers passed in (PyTorch-ROCm allocations passed as raw device pointers); all device work
 * is enqueued on the caller's HIP stream (hipStream_t passed as void*) and nothing synchronises
 * except bp_load_scenarios and the bp_get_* / bp_check_errors host copies; a handle is bound to one
 * device and is not thread-safe.  Physics arithmetic is IEEE binary64 ("f64").
 */
#ifndef BENCHPUSH_AMD_H
#define BENCHPUSH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BP_ABI_VERSION 11
#define BP_MAXV 20          /* max hull vertices per shape (generate_polygon draws 10-20, polygon.py:53,72) */
#define BP_MAX_SHIP_VERTS 32
#define BP_OBS_C 4
#define BP_INFO_COUNT 16

enum {
    BP_OK = 0,
    BP_EINVAL = -1,      /* bad argument / unsupported configuration */
    BP_ENOMEM = -2,
    BP_EHIP = -3,        /* HIP runtime error, see bp_last_error */
    BP_ENODEVICE = -4,   /* no usable GPU: the product path refuses to run without one */
    BP_ESTATE = -5,      /* call order violated (e.g. step before load/reset) */
    BP_ECAPACITY = -6    /* an in-kernel capacity (neighbour list / arbiter slots) overflowed */
};

enum { BP_ENV_SHIP_ICE = 0, BP_ENV_MAZE = 1, BP_ENV_BOX = 2 };
#define BP_MAX_WHEELS 4

/* per-env error bits reported by bp_check_errors */
enum { BP_ERR_ADJ_OVERFLOW = 1, BP_ERR_ARB_OVERFLOW = 2, BP_ERR_LEVEL_OVERFLOW = 4,
       BP_ERR_SCHED_TIMEOUT = 8 /* a scheduler fault left more envs unfinished than the completion launch can finish (256): the step is incomplete;
                                   smaller faults are finished by the completion launch and counted by bp_sched_warnings (ABI 7) */ };

/* info[e][k] columns written by bp_step / bp_reset (ship_ice_env.py:337-345 plus the callback
 * bookkeeping of :150-180); state is raw (the host adapter applies round(.,2)). */
enum {
    BP_I_X = 0, BP_I_Y, BP_I_THETA, BP_I_TOTAL_WORK, BP_I_WORK, BP_I_COLL_REWARD, BP_I_SCALED_COLL,
    BP_I_DIST_REWARD, BP_I_SUCCESS, BP_I_BOUNDARY, BP_I_YAW, BP_I_KE, BP_I_IMPULSE, BP_I_NPOST,
    BP_I_NCONTACT, BP_I_NFIRST
};

/* Scalar configuration (ship_ice_nav/config.yaml + constants of ship_ice_env.py, see
 * benchpush_amd/config.py:ship_ice_physics_params for the file:line of each). */
typedef struct bp_config {
    double dt;               /* env step (s) */
    int32_t steps;           /* physics sub-steps per env step */
    int32_t iterations;      /* solver iterations */
    int32_t persistence;     /* Chipmunk collision_persistence */
    int32_t settle_steps;    /* sub-steps run by reset */
    double damping_pow;      /* pow(space.damping, dt/steps), in [0, 1] (ship_ice_env.py:120, maze_NAMO_env.py:148: space.damping = cfg.sim.damping).
                              * 0 (every shipped config) runs the specialised kernels; any other value selects a generic instantiation of the same
                              * sub-step (k_physics_step_damp: velocities scaled instead of cleared, moving list rebuilt from the velocity slots,
                              * no step scheduler) -- slower, and bodies once pushed keep moving, so the in-kernel capacities (BP_ECAPACITY) are
                              * reached sooner.  The same holds for box-delivery / area-clearing handles (bp_bd_config.damping_pow, box_delivery_env.py:204: k_bd_settle_damp /
                              * k_bd_physics_damp). */
    double bias_coef;        /* 1 - pow(collision_bias, dt/steps) */
    double slop;
    double target_speed;
    double max_yaw_rate;
    double map_w, map_h;
    double goal_y;
    double m_to_pix;
    double density;
    double poly_radius;
    double elasticity;
    double friction;
    double beta;
    double boundary_penalty;
    double terminal_reward;
    double local_w, local_h;
    double vshift;
    double obs_range;
    int32_t num_ship_verts;
    int32_t _pad;
    double ship_verts[BP_MAX_SHIP_VERTS][2];  /* cfg.ship.vertices */
    double ship_head[2], ship_tail[2];
    /* ---- maze-NAMO-v0 (benchpush/environments/maze_NAMO/maze_NAMO_env.py, config.yaml); ignored for ship-ice ---- */
    int32_t env_kind;        /* BP_ENV_SHIP_ICE | BP_ENV_MAZE; for the maze ship_verts holds cfg.robot.vertices and map_w/map_h
                                hold cfg.env.width/length, goal_y cfg.env.goal_y */
    int32_t num_wheels;      /* cfg.robot.wheel_vertices (4 quads) */
    double wheel_verts[BP_MAX_WHEELS][4][2];
    double goal_x;           /* cfg.env.goal_x */
    double goal_reach;       /* cfg.goal_radius + cfg.robot.min_r, maze_NAMO_env.py:528-536 */
    double k_increment;      /* 150, maze_NAMO_env.py:82 */
    double wall_radius;      /* 0.5, sim_utils.py:177 */
    double obstacle_size;    /* cfg.obstacle_size */
    /* ---- ship-ice: per-episode start pose and metric constants ---- */
    int32_t random_start;    /* cfg.random_start (ship_ice_env.py:201-203): start = (1 + u * (start_x_range - 1), 1.0, pi/2) with u drawn per
                                (env, episode) from a counter RNG instead of python's global `random` (bp_start_uniform below); every reset
                                then re-runs the settle sub-steps, because the settled field depends on where the ship sits */
    int32_t _pad2;
    double start_x_range;    /* cfg.start_x_range */
    uint64_t start_seed;     /* key of the counter RNG */
    double ship_mass;        /* cfg.ship.mass: m0 of ShipIceMetric.compute_effort_score (ship_ice_metric.py:62-69) */
} bp_config;

/* The uniform in [0, 1) that bp_reset draws for (global env id, episode index) when random_start is set: the top 53 bits of
 * splitmix64(seed ^ splitmix64(global_env_id * 2^32 + episode)) / 2^53.  Exposed so that callers (and the parity tests) can
 * reproduce start poses on the host. */
double bp_start_uniform(uint64_t seed, int64_t global_env_id, int64_t episode);

typedef struct bp_handle bp_handle;

/* Create a handle for `num_envs` environments on HIP device `device`.  `env_id_offset` is the global id
 * of local env 0 (multi-GPU sharding: rank r owns [r*E/R, (r+1)*E/R)); trial selection uses the global id.
 * Replaces ShipIceEnv.__init__ (ship_ice_env.py:37-106). */
int bp_create(const bp_config *cfg, int32_t num_envs, int64_t env_id_offset, int32_t device, bp_handle **out);
int bp_destroy(bp_handle *h);

/* Upload `num_trials` ice fields (host pointers).  verts[T][F][V][2] raw world-space polygon vertices as stored in
 * the reference's trial dicts ('vertices'), counts[T][F] vertex counts (0 = unused slot), centres[T][F][2]
 * ('centre'), starts[T][3] ship start pose, nfloes[T].  Performs the body/shape construction of
 * sim_utils.py:136-163 + ship.py:77-98 (convex hull, COG recentre, mass/moment from density) on the host and
 * copies SoA arrays to the device.  Replaces the pickle load of ship_ice_env.py:76-80 and init_ship_ice_env :186-216. */
int bp_load_scenarios(bp_handle *h, int32_t num_trials, int32_t F, int32_t V, const double *verts,
                      const int32_t *counts, const double *centres, const double *starts, const int32_t *nfloes);

/* maze-NAMO-v0 counterpart of bp_load_scenarios: `num_layouts` box layouts (host pointers), centres[T][nbox][2], the wall
 * segments walls[nwalls][4] = ax, ay, bx, by (construct_maze_walls, maze_NAMO_env.py:357-375) and the start poses start[num_layouts][3]
 * (the fixed pose of :241-245, or one draw of cfg.random_start per layout, :229-238).  Builds the
 * KINEMATIC robot (body + wheels, robot.py:77-118), the boxes (sim_utils.py:136-163), the static Segment(radius 0.5) walls
 * (sim_utils.py:174-181) and the BFS goal map (occupancy_map.py:435-485) on the host.  Replaces init_maze_NAMO_env (:221-269). */
int bp_load_maze(bp_handle *h, int32_t num_layouts, int32_t nbox, const double *centres, int32_t nwalls, const double *walls,
                 const double *start);
/* maze: goal map as the reference returns it in info['goal_dt'] (un-normalised wavefront distances), host double [grid_h][grid_w] */
int bp_get_goal_map(bp_handle *h, double *out_host, int32_t *grid_h, int32_t *grid_w);

/* reset() for the envs whose env_mask byte is non-zero (device pointer; NULL = all envs): next trial
 * ((global_env_id + episode_idx) % num_trials), new space, 1000 settle sub-steps, first observation.
 * obs: device uint8 [E][4][H][W] (rows of unmasked envs untouched); info: device double [E][BP_INFO_COUNT] or NULL.
 * Replaces ShipIceEnv.reset (ship_ice_env.py:223-249). */
int bp_reset(bp_handle *h, const uint8_t *env_mask, uint8_t *obs, double *info, void *stream);

/* One env.step() for every env: actions device double [E] in [-1,1]; obs device uint8 [E][4][H][W]; reward device
 * double [E]; terminated / truncated device uint8 [E]; info device double [E][BP_INFO_COUNT] (may be NULL).
 * Replaces ShipIceEnv.step (ship_ice_env.py:261-355): 400 x pymunk.Space.step, work, reward, raster. */
int bp_step(bp_handle *h, const double *actions, uint8_t *obs, double *reward, uint8_t *terminated,
            uint8_t *truncated, double *info, void *stream);

/* reset() copies a per-trial template that was settled once at load time (the reference's reset is a pure function of
 * the trial when cfg.random_start is off); on != 0 re-runs the settle sub-steps in place instead (identical result). */
int bp_set_resettle(bp_handle *h, int32_t on);

/* Physics only / raster only halves of bp_step (profiling and tests). */
int bp_step_physics(bp_handle *h, const double *actions, double *reward, uint8_t *terminated, uint8_t *truncated,
                    double *info, void *stream);
int bp_observe(bp_handle *h, const uint8_t *env_mask, uint8_t *obs, void *stream);

/* Planner observation of ship-ice (cfg.egocentric_obs: false, ship_ice_env.py:96-99,394-406): device uint8
 * [E][2][map_h/0.2][map_w/0.2] = [5x5 block-mean occupancy of every floe, ship footprint on the 0.2 m grid]. */
int bp_observe_global(bp_handle *h, const uint8_t *env_mask, uint8_t *obs, void *stream);

/* Planner cost map of ship-ice: CostMap.__init__ / boundary_cost / update / populate_costmap of
 * benchpush/common/cost_map.py:27-126,284-287 evaluated on the environments' current obstacles (what the planners pass as
 * info['obs'], lattice.py:78-79).  out: device double [E][(int)(m*scale)][(int)(n*scale)].  ship_pos_y: device double [E] in
 * cost-map units (the planner passes ship_y*scale - max_ship_length/2) or NULL for 0; horizon <= 0 means horizon=None. */
typedef struct bp_costmap_config {
    double scale;       /* cells per metre (lattice_config.yaml:43) */
    int32_t m, n;       /* channel height / width in metres */
    double alpha;       /* collision cost weight */
    double ship_mass;
    double horizon;     /* metres ahead of ship_pos_y that are considered; <= 0: everything */
    int32_t margin;     /* boundary columns set to 1e10 */
    int32_t pad_;
} bp_costmap_config;
int bp_costmap_update(bp_handle *h, const bp_costmap_config *cfg, const double *ship_pos_y, double vs, double *out, void *stream);

/* info['obs'] (cost_map.py:275-281): world-space hull vertices of every shape, device double [E][nb_cap][BP_MAXV][2],
 * counts device int32 [E][nb_cap] (index 0 = ship, then floes in trial order). */
int bp_get_world_polys(bp_handle *h, double *out, int32_t *counts, void *stream);
/* body state, device double [E][nb_cap][9] = x, y, angle, vx, vy, w, v_bias.x, v_bias.y, w_bias */
int bp_get_body_state(bp_handle *h, double *out, void *stream);
/* low-dimensional observation (ship_ice_env.py:358-370): |centroid| of every floe, device double [E][nb_cap-1][2] */
int bp_get_low_dim_obs(bp_handle *h, double *out, void *stream);

/* Per-episode metrics accumulated on the device (all four environments; box-delivery and area-clearing handles: see below; the maze uses MazeNamoMetric's L = wavefront length at the
 * start pixel, maze_namo_metric.py:68-75, and bp_config.ship_mass = cfg.robot.mass): what ShipIceMetric.update / reset keep per episode
 * (benchpush/common/metrics/ship_ice_metric.py:26-69, base_metric.py:12-16) -- summed reward, path length of the ship integrated from
 * the state rounded to 2 decimals like info['state'] (ship_ice_env.py:337-339), total_work, success, steps -- updated by every bp_step /
 * bp_reset.  When an env terminates (or is reset while its episode is still running: eps_complete by truncation) its row is written:
 *   rows   device double [E][BP_EPM_COUNT] = efficiency, effort, episode reward, success, episode length (steps), total_work
 *          of the env's most recently finished episode,
 *   counts device uint32 [E] episodes finished so far.
 * [E][6] is the block that crosses GPUs (one all-gather per evaluation batch). */
#define BP_EPM_COUNT 6
enum { BP_EPM_EFFICIENCY = 0, BP_EPM_EFFORT, BP_EPM_REWARD, BP_EPM_SUCCESS, BP_EPM_LENGTH, BP_EPM_TOTAL_WORK };
int bp_get_episode_metrics(bp_handle *h, double *rows, uint32_t *counts, void *stream);
/* The episode LISTS that BaseMetric keeps (base_metric.py:12-16: one entry per finished episode), without a host round trip per step:
 *   ring   device double [E][BP_EPM_RING][BP_EPM_COUNT]: episode n of an env (n = 0, 1, ...) is in slot n % BP_EPM_RING, so the last BP_EPM_RING
 *          finished episodes of every env are available in order,
 *   sums   device double [E][BP_EPM_COUNT]: the six row fields summed over ALL finished episodes of the env (the means of an evaluation are
 *          sums / counts; [E][7] with the count is the block that crosses GPUs),
 *   counts device uint32 [E] episodes finished so far.  Any pointer may be NULL. */
#define BP_EPM_RING 8
int bp_get_episode_history(bp_handle *h, double *ring, double *sums, uint32_t *counts, void *stream);
/* Box-delivery and area-clearing handles keep the reference's TaskDrivenMetric (benchpush/common/metrics/task_driven_metric.py) in the same rows, updated
 * by bp_step / bp_reset / bp_bd_step_async / bp_bd_async_drain (an asynchronous call accounts only the envs whose ready byte it set):
 *   efficiency = mst_cost / l0, effort = (m0 l0 + sum_i d_i area_i) / (m0 l0 + total_work) over the completed boxes i, episode reward,
 *   success = completed boxes / boxes (a rate), steps, total_work -- l0 the path length of the robot position rounded to 2 decimals, m0 =
 *   bp_bd_config.robot_mass, d_i the distance from box i's centroid AT RESET to the nearest goal (receptacle position / boundary goal points), mst_cost the
 *   minimum spanning tree over the completed boxes' reset centroids, their goals and the robot start.  0 / 0 and x / 0 are IEEE (NaN, inf).
 * bp_bd_get_episode_boxes: device double [E][24][3] = area, cx, cy of every box polygon as it stood after the env's last reset (zeros in unused slots);
 * BP_EINVAL for handles of the other environments. */
int bp_bd_get_episode_boxes(bp_handle *h, double *out_device, void *stream);
/* info['box_completed_statuses'] of every env as the metric reads it: host uint8 [E][24], 1 = box k is delivered (box-delivery: no longer alive) / cleared
 * (area-clearing), 0 otherwise and in unused slots (synchronises).  BP_EINVAL for handles of the other environments. */
int bp_bd_get_completed(bp_handle *h, uint8_t *out_host);
/* The row arithmetic of those handles as a pure host function (no GPU, no handle; the code the kernel runs): boxes_acxy [nbox][3] = area, cx, cy;
 * completed uint8 [nbox]; goals_xy [ngoal][2]; start_xy [2]; robot_dist = l0; out6 = the BP_EPM_* columns.  Returns 0, or -1 for a null pointer, nbox outside
 * 0 .. 24 or ngoal < 1. */
int bp_task_metric_row(int32_t nbox, const double *boxes_acxy, const uint8_t *completed, int32_t ngoal, const double *goals_xy, const double *start_xy,
                       double robot_mass, double robot_dist, double total_work, double reward, double steps, double *out6);
/* Rollout plumbing for vectorised callers (the reference's learners wrap the env in SB3's VecEnv, whose auto-reset hands the LAST observation of a
 * finished episode back as infos[i]['terminal_observation'], baselines/ship_ice_nav/ppo/policy.py:29-69): copies row r of src to row r of dst for every r with
 * mask[r] != 0 -- device pointers, rows of row_bytes bytes (a multiple of 4), nothing is read back, so the caller can save the observations of the envs that are
 * about to be reset without a host synchronisation.  Cost is proportional to the rows selected.  ABI 9. */
int bp_copy_rows_masked(bp_handle *h, const uint8_t *mask, const void *src, void *dst, int64_t rows, int64_t row_bytes, void *stream);
/* test hook: out[i] = the device's restatement of python's round(in[i], 2) (device doubles [n]) */
int bp_debug_round2(const double *in_dev, double *out_dev, int32_t n, void *stream);
/* test hook: overwrite every cached-plane hint word of the live envs with random valid contents (indices below the recorded vertex counts, random
 * flags); the following steps must produce bit-identical results -- the hints only steer how much of the plane search is skipped.
 * Returns the number of words rewritten (>= 0) or a negative BP_E*; synchronises the stream. */
int bp_debug_scramble_hints(bp_handle *h, uint64_t seed, void *stream);

int32_t bp_nb_cap(const bp_handle *h);       /* body slots per env (ship + max floes, padded) */
int32_t bp_obs_height(const bp_handle *h);
int32_t bp_obs_width(const bp_handle *h);
/* number of bodies (ship + floes) currently in each env: host int32 [E] (synchronises) */
int bp_get_num_bodies(bp_handle *h, int32_t *out_host);
/* Copies per-env error bits to host int32 [E] (may be NULL) and returns BP_ECAPACITY if any is set (synchronises). */
int bp_check_errors(bp_handle *h, int32_t *out_host);
/* kernel timing helper for bench.py: average duration (ms) of the physics kernel over launches since the last call,
 * measured with HIP events on the launch stream (synchronises). */
int bp_kernel_time_ms(bp_handle *h, double *physics_ms, double *raster_ms, int32_t *launches);
int bp_enable_timing(bp_handle *h, int32_t on);
/* Per-launch cost statistics of the bp_step calls since bp_enable_timing(h, 1) (ship-ice and maze handles, at most 1024 launches): out_host[k][0] = sum
 * over the envs of the shader cycles >> 8 their wavefronts spent in launch k, out_host[k][1] = the largest of them.  With the clock of the run they give
 * the two lower bounds of a launch -- all work packed into the device's wave slots, and the busy time of the heaviest env (bench.py roofline.ceiling).
 * Host uint64 [max_launches][2]; *launches = rows written (synchronises).  ABI 11. */
int bp_get_cost_stats(bp_handle *h, uint64_t *out_host, int32_t max_launches, int32_t *launches);
/* shader cycles >> 8 each env's wavefront spent in the last bp_step (the dispatch-order hint): host uint32 [E] (synchronises) */
int bp_get_step_cycles(bp_handle *h, uint32_t *out_host);
/* sub-steps per chunk of the preemptive step scheduler (k_physics_step_sched: envs are parked at chunk boundaries while another one is further
 * behind, and resumed by another workgroup; results are identical), 0 = one wavefront per env for the whole step.  Default 40 for ship-ice and
 * maze handles of up to 8192 envs; environment variable BP_SCHED=<chunk> (0 = off) overrides it at load time. */
int32_t bp_sched_chunk(bp_handle *h);
/* Resident wavefronts of the step scheduler (k_physics_step_schedl: one workgroup per wave slot of the device takes task after task itself instead of one
 * workgroup per task from the hardware dispatcher; results are identical): the number of resident workgroups of a scheduled launch, 0 = one workgroup per
 * task.  Default: 8 x the device's compute units for scheduled launches (k_physics_step_schedr in pairing launches); environment variables BP_SCHED_PERSIST=0 /
 * BP_PAIR_RESIDENT=0 turn it off.  (ABI 10)  A resident kernel holds every wave slot for the whole launch, which suits one process per GPU only: unless one of
 * the two variables is set, the handle checks every 64 launches whether another PROCESS has a resident handle on the same device (advisory lock on
 * $BP_LOCK_DIR|/tmp/benchpush_amd.resident.<pci bus id>.lock) and launches the dispatcher-driven kernels while that is so; the value returned is that of the
 * launches being issued now (0 while the device is shared).  bp_device_shared: 1 while the last check saw another process.  (ABI 11) */
int32_t bp_sched_resident(bp_handle *h);
int32_t bp_device_shared(bp_handle *h);
/* The load-time launch policy as a pure function (no GPU, no handle): regime boundaries are rounds of the device's wave slots (8 per compute unit), not env
 * counts -- pairing from 2.5 rounds, loose pairing limits from 3.5, no scheduler without pairing above 4 (5 120 / 7 168 / 8 192 envs on the 256 CUs of an
 * MI355X).  out8_host = wave slots, pair mode (0 / 2), tight limits (0 / 1), envs that start alone, sub-steps per scheduler chunk (0 = no scheduler), and
 * the three leave limits (active arbiters, work units per sub-step, work rate).  (ABI 11) */
int bp_launch_policy_query(int32_t num_envs, int32_t num_compute_units, int32_t can_pair, int32_t is_maze, int32_t *out8_host);
/* Two environments per wavefront (ship-ice handles with space.damping == 0 and at most 448 body slots (PP_NBCAP); lanes 0..31 one env, lanes 32..63 another, results
 * identical): 0 = off, 1 = fixed pairs of the dispatch order for the whole step (test kernel), 2 = inside the step scheduler: the heaviest envs of the
 * dispatch order start alone, the others in pairs, and an env that outgrows the half-wave capacities or turns heavy is parked at a sub-step boundary and
 * resumed in a wavefront of its own.  Environment variable BP_PAIR=<mode> selects it at load time.  ABI 9. */
int32_t bp_pair_mode(bp_handle *h);
/* Parameters and cumulative counters of the pairing (host int32 [16], synchronises): [0..7] = mode, envs of the dispatch order that start alone, and the
 * limits above which an env leaves its pair (arbiter lanes, velocity slots, moving bodies, active arbiters, warm arbiters x colours, work proxy per
 * sub-step); [8..15] = since load: paired first tasks, paired tasks formed from the queues, envs that finished their step in a pair, envs that left a pair
 * as heavy and carried on alone in the same wave slot, heavy envs queued, light envs queued (mates of split pairs and yields), -, -.  ABI 9. */
int bp_get_pair_stats(bp_handle *h, int32_t *out16_host);
/* Clock calibration for bench.py: the shader-clock counter (s_memtime) and the 100 MHz reference counter (s_memrealtime) stamped on the device right
 * after every physics launch of bp_step / bp_reset (ship-ice and maze handles) by one thread, filed under the XCD it ran on (the shader-clock counters
 * of different XCDs are not synchronised): out[x][0..1] = the latest pair taken on XCD x, zeros if none yet.  The clock the chip held between two
 * calls is (d out[x][0]) / (d out[x][1]) x 100 MHz for any x stamped before the first and before the second call (MI355X_MICROARCH.md, DVFS item 6).
 * Host uint64 [8][2] (synchronises).  ABI 8 (ABI 7: one pair, whatever the XCD). */
int bp_get_clock_stamps(bp_handle *h, uint64_t *out16_host);
/* Scheduler robustness counters since bp_load_*: out2_host[0] = launches in which the watchdog of the step scheduler fired (a workgroup gave up
 * waiting for a parked env -- a scheduler fault, never seen in practice), out2_host[1] = envs whose step the completion launch that follows every
 * scheduled launch had to finish.  Results are complete and identical either way; non-zero values are a warning, not an error (synchronises). */
int bp_sched_warnings(bp_handle *h, int32_t *out2_host);
/* overrides that hint for the next bp_step: host uint32 [E], larger = dispatched earlier (results never depend on the order; synchronises) */
int bp_set_step_cost_hint(bp_handle *h, const uint32_t *host_costs);

/* ---------------------------------------------------------------------------------------------------------------
 * box-delivery-v0 (benchpush/environments/box_delivery/box_delivery_env.py, config.yaml).  A handle made by bp_bd_create is
 * (task 0) is driven by the same bp_reset / bp_step / bp_observe / bp_get_body_state / bp_check_errors / bp_destroy entry points:
 *   actions  device double [E]: 'heading' action in [-1, 1] (box_delivery_env.py:706-723) or 'position' index into the local map;
 *            device double [E][2] = (linear, angular) speed for 'velocity' (:672-703), selected by bp_bd_config.action_type
 *   obs      device uint8 [E][local_px][local_px][4], channels last (box_delivery_env.py:1045-1059)
 *   info     device double [E][BP_INFO_COUNT]: BP_BD_I_* columns
 * Replaces BoxDeliveryEnv.step (:634-830: PositionController waypoints, execute_robot_path, step_simulation_until_still,
 * spfa-based box distances, rewards, receptacle removal) and generate_observation (:1045-1207).
 * --------------------------------------------------------------------------------------------------------------- */
enum {
    BP_BD_I_X = 0, BP_BD_I_Y, BP_BD_I_THETA, BP_BD_I_CUM_DIST, BP_BD_I_CUM_BOXES, BP_BD_I_CUM_REWARD, BP_BD_I_TOTAL_WORK,
    BP_BD_I_MINISTEPS, BP_BD_I_INACTIVITY, BP_BD_I_HIT, BP_BD_I_SUBSTEPS, BP_BD_I_ROBOT_DIST, BP_BD_I_BOXES_DIST, BP_BD_I_NWP,
    BP_BD_I_NALIVE, BP_BD_I_WORK
};
typedef struct bp_bd_config {
    double ctrl_dt;                    /* controller.dt (config.yaml:43); one sim step is ctrl_dt / steps */
    int32_t steps, iterations, persistence, settle_steps;   /* sim.steps, sim.iterations, Chipmunk persistence 3, 1000 (:284) */
    double damping_pow, bias_coef, slop;                     /* as in bp_config */
    double room_length, room_width;    /* env.room_length, env.room_width_small|large */
    double recept_x, recept_y, recept_size;                  /* get_receptacle_position_and_size (:322-324) */
    double ppm;                        /* local_map_pixel_width / local_map_width */
    double local_w;                    /* env.local_map_width */
    int32_t local_px;                  /* env.local_map_pixel_width */
    int32_t use_correct_direction_reward;
    double robot_radius, robot_half_width;                   /* :122-123 */
    double step_size, target_speed;    /* agent.step_size, controller.target_speed */
    double partial_rewards_scale, goal_reward, collision_penalty, non_movement_penalty, correct_direction_reward_scale;
    double ministep_size, sp_channel_scale;
    int32_t inactivity_cutoff, invert_receptacle_map, num_boxes, step_limit;
    int32_t action_type;               /* agent.action_type: 0 heading, 1 position, 2 velocity */
    int32_t task;                      /* 0 box-delivery-v0; 1 area-clearing-v0 (environments/area_clearing/area_clearing.py:611-778) */
    double omega_scale, v_scale, lfc;  /* apply_controller factors (3, 2 | 0.5, 5) and the DP look-ahead controller.Lfc (0 | 0.5) */
    /* area-clearing only: velocity action scale, sim.t_max, the reward constants of area_clearing.py:37-49, DISTANCE_SCALE_MAX */
    double yaw_rate_step;
    int32_t t_max, num_goal_points, num_boundary_verts, num_outer_verts;
    double boundary_penalty, box_cleared_reward, box_putback_penalty, truncation_penalty, terminal_reward, pushing_mult, distance_scale_max;
    double boundary[8][2], outer_boundary[8][2];   /* env_cfg.boundary / outer_boundary (convex polygons) */
    double footprint_verts[4][2];                  /* agent.footprint_vertices */
    double goal_points[128][2];                    /* _compute_boundary_goals (:225-264) */
    double box_half, box_density;      /* boxes.box_size / 2, boxes.box_density */
    double robot_verts[4][2];          /* agent.vertices */
    double wheel_verts[4][4][2];       /* agent.wheel_vertices */
    double bumper_verts[4][2];         /* agent.front_bumper_vertices */
    double robot_mass;                 /* agent.mass: m0 of the episode metrics (TaskDrivenMetric); last member, added within ABI 11 */
} bp_bd_config;
/* area-clearing-v0 uses the same entry points with bp_bd_config.task = 1: heading/position/velocity actions, obs uint8
 * [E][224][224][4], info columns = x, y, theta, total_work, collision reward, diff_reward, box_completed_reward, box_count, ministeps,
 * robot_hit_obstacle, sim steps, robot distance, t, #waypoints, work, pushing reward.  bp_bd_load then takes no receptacle polygon;
 * static polygons (walls radius 0.1) get pymunk's default elasticity 0 and friction 0.99 (area_clearing.py:446-474).
 * Replaces AreaClearingEnv.step / reset / generate_observation (:563-778,927-1120). */
int bp_bd_create(const bp_bd_config *cfg, int32_t num_envs, int64_t env_id_offset, int32_t device, bp_handle **out);
/* `num_trials` episodes (host pointers): starts[T][3] robot start pose, boxes[T][nbox][3] = x, y, heading, and `nstatic` static
 * polygons per trial in generate_sim_bounds order (sim_utils.py:90-135): sverts[T][ns][4][2], scount[T][ns] (3 or 4 vertices),
 * spose[T][ns][3] body x, y, angle, srad[T][ns] shape radius, stype[T][ns] collision type (3 obstacle, 4 receptacle; exactly one
 * receptacle; scount 0 = unused padding slot when trials hold different numbers of columns).  Builds bodies/shapes (sim_utils.py:20-160), the configuration space, nearest-free-cell indices and the
 * receptacle distance map (box_delivery_env.py:1115-1175) on the host, settles every trial once.
 * Replaces init_box_delivery_sim / init_box_delivery_env (:193-292). */
int bp_bd_load(bp_handle *h, int32_t num_trials, int32_t nbox, const double *starts, const double *boxes, int32_t nstatic,
               const double *sverts, const int32_t *scount, const double *spose, const double *srad, const int32_t *stype);
int32_t bp_bd_sizeof_config(void);
/* tests: static rasters of trial t over the small-map window, host buffers (any may be NULL): dims[6] = H, W, SH, SW, si0, sj0;
 * cspace / cspace_thin uint8 [SH][SW]; edt uint16 [SH][SW][2]; recept float [SH][SW]; small_free uint8 [SH][SW] */
int bp_bd_get_maps(bp_handle *h, int32_t trial, int32_t *dims, uint8_t *cspace, uint8_t *cspace_thin, uint16_t *edt, float *recept,
                   uint8_t *small_free);
/* Two-pass step of box-delivery / area-clearing handles (ABI 9): out2_host[0] = env steps whose sim-step loop ran past the budget of the first pass and was
 * finished by the second one (beside the finish / map / observation kernels of all other envs), out2_host[1] = env steps whose execute_robot_path or
 * step_simulation_until_still loop ran into STEP_LIMIT (box_delivery_env.py:62,891-1023) -- cumulative since load (host uint32 [2], synchronises).
 * BP_BD_BUDGET=<sim steps> sets the budget of the first pass at load time (default 3000; 0 = one pass); bp_bd_budget returns the value the handle uses (ABI 11). */
int bp_bd_get_stragglers(bp_handle *h, uint32_t *out2_host);
int32_t bp_bd_budget(bp_handle *h);
/* Exact recurrences of execute_robot_path (box_delivery_env.py:891-988; ABI 11): while only the robot moves and no arbiter exists, a sim step is a function of the
 * robot's parts and the controller's loop variables; when that state is bit for bit the one of p sim steps ago (a robot that pushes against a wall until
 * STEP_LIMIT sits at a fixed point, p = 1, within a few hundred sim steps) whole periods are skipped -- results, sim-step counts and info columns are
 * those of the full loop.  out2_host[0] = recurrences found, out2_host[1] = sim steps they skipped, cumulative since load (host uint32 [2], synchronises).
 * The test runs in the second pass of the two-pass step (k_bd_physics_resume: the envs that ran out of the first pass's sim-step budget, BP_BD_BUDGET -- the kernel every
 * env runs stays lean); BP_BD_CYCLE=<n> at load time: only once a path has run n sim steps, 0: every sim step is run. */
int bp_bd_get_cycle_skips(bp_handle *h, uint32_t *out2_host);
/* Asynchronous step of box-delivery / area-clearing handles (opt-in; bp_step is unchanged).  Every env is idle or busy, busy = in the middle of an env step
 * with its loop state on the device.  bp_bd_step_async: an idle env takes its row of `actions` (shaped as for bp_step), is planned and starts an env step; a
 * busy env ignores its row and resumes; every env then runs at most `budget` >= 1 sim steps.  An env whose env step ends in the call writes its rows of obs /
 * reward / terminated / truncated / info exactly as bp_step does, gets ready[e] = 1 and slices[e] = the number of calls the env step took, and is idle again;
 * every other env gets ready[e] = 0, its rows (slices[e] included) are not touched, and its env step continues in the next call.  ready is uint8 [E], slices
 * int32 [E], both on the device.  The transitions an env emits are those of bp_step for the actions it accepted, bit for bit, whatever the budget, the other
 * envs or the cut of the calls.  bp_bd_async_drain runs the busy envs, and only those, to the end of their env steps (same outputs; idle envs emit nothing)
 * and closes the slice.  While a slice is open -- from a bp_bd_step_async to a drain or a bp_reset of all envs (env_mask NULL) -- bp_step, bp_step_physics,
 * bp_save_state, bp_load_state and bp_clone_state return BP_ESTATE with nothing touched (state records do not carry the loop state); bp_reset with a mask
 * cancels the busy envs of the mask (no transition for the half-done env step) and starts their next trials as usual; read-only calls show a busy env
 * mid-step.  bp_bd_async_open returns 1 while a slice is open (a host flag).  Nothing synchronises; all work is enqueued on `stream`.
 * BP_EINVAL: NULL handle or tensor (obs may be NULL: no observations), budget < 1, a handle of another environment, or one with damping != 0;
 * BP_ESTATE before load and reset.  (Added within ABI 11: the additions only add.) */
int bp_bd_step_async(bp_handle *h, const double *actions, int32_t budget, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
                     double *info, uint8_t *ready, int32_t *slices, void *stream);
int bp_bd_async_drain(bp_handle *h, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated, double *info, uint8_t *ready,
                      int32_t *slices, void *stream);
int32_t bp_bd_async_open(bp_handle *h);
/* Ready queue of the asynchronous step: fixed-size recv / send batches, the queue between the two on the device (opt-in; the calls above are unchanged).
 * With a queue open every env is idle (has an action, starts in the next recv), busy, or held: it emitted a transition or was reset and waits in the queue
 * or for its send.  The queue is a FIFO ring of env ids with capacity E; an env is in it at most once.  Its order is a function of the handle's history
 * alone: enqueue events (open, recvs, sends) in stream order, ascending env id within one event.
 *   bp_bd_queue_open(batch = M, 1 <= M <= E): needs a handle that was reset and has no open slice.  Every env becomes held and is queued, in env-id order,
 *     as a fresh row: its current observation and info row, no transition.  Opens the slice (bp_bd_async_open is 1).
 *   bp_bd_queue_recv(budget >= 1, flags): one slice call exactly as bp_bd_step_async launches it, writing the [E] rows obs_e / reward_e / terminated_e /
 *     truncated_e / info_e / slices_e of the envs that emitted and emitted[E] (that call's ready mask); then the envs that emitted are appended in ascending
 *     env id and become held, up to M ids leave the head into ids[M] (int32), and row j of obs [M][rows of obs_e] / reward [M] / terminated [M] /
 *     truncated [M] / info [M][BP_INFO_COUNT] / slices [M] gets the rows of env ids[j].  A fresh row has reward 0, flags 0 and slices 0; rows beyond the
 *     count have ids[j] = -1 and zeros.  counts (int32 [5]): rows delivered, ids still queued, busy envs, envs taken and not sent yet (these rows included),
 *     rejected send rows so far.  With BP_QUEUE_FULL_ONLY in flags nothing is taken (count 0) while fewer than M ids are queued and an env is still
 *     busy: a caller that wants full batches repeats the call.  obs_e and obs may both be NULL (no observations); otherwise a row is a multiple of 16 bytes and both are 16-byte aligned.
 *   bp_bd_queue_send(actions [M][action dim], ids [M], reset [M] or NULL): row j with ids[j] >= 0 hands env ids[j] its next action -- the env is idle and starts
 *     in the next recv -- or, with reset[j] != 0, resets it as bp_reset with a mask does (next trial, the episode closes in the episode metrics; obs_e /
 *     info_e get the rows) and queues it as a fresh row, reset rows of one send in ascending env id; the env stays held.  Rows with ids[j] == -1 are ignored.
 *     A row is rejected -- ignored, and counted in counts[4] -- if its env is not taken and awaiting its send (out of range, busy, idle, still queued) or if a
 *     smaller row of the same send names the same env.  reset == NULL launches no reset kernel.
 *   bp_bd_queue_close: the drain (the busy envs finish, outputs as bp_bd_async_drain), then the queue is discarded, every env is idle and the slice is closed.
 *     A bp_reset of all envs closes the queue too, without the drain.
 *   bp_bd_queue_batch: M while a queue is open, else 0 (a host flag).
 * While a queue is open bp_bd_step_async, bp_bd_async_drain and bp_reset with a mask return BP_ESTATE like the calls an open slice refuses; nothing is launched.
 * State records carry neither queue nor loop state.  Nothing synchronises and nothing is read back; all work is enqueued on `stream`; all tensors are device
 * memory.  BP_EINVAL: NULL handle or tensor, batch outside [1, E], budget < 1, a handle of another environment or one with damping != 0; BP_ESTATE: before
 * load and reset, open on an open slice, recv / send / close without a queue.  A recv that fails part-way leaves the handle open and refusing, as
 * bp_bd_step_async.  (Added within ABI 11: the additions only add.) */
int bp_bd_queue_open(bp_handle *h, int32_t batch, void *stream);
#define BP_QUEUE_FULL_ONLY 1   /* bp_bd_queue_recv flags: take nothing while fewer than M ids are queued and an env is still busy */
int bp_bd_queue_recv(bp_handle *h, int32_t budget, int32_t flags, uint8_t *obs_e, double *reward_e, uint8_t *terminated_e, uint8_t *truncated_e, double *info_e,
                     uint8_t *emitted, int32_t *slices_e, int32_t *ids, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated,
                     double *info, int32_t *slices, int32_t *counts, void *stream);
int bp_bd_queue_send(bp_handle *h, const double *actions, const int32_t *ids, const uint8_t *reset, uint8_t *obs_e, double *info_e, void *stream);
int bp_bd_queue_close(bp_handle *h, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated, double *info, uint8_t *ready, int32_t *slices,
                      void *stream);
int32_t bp_bd_queue_batch(bp_handle *h);
/* tests: per-env box bookkeeping, host buffers: alive uint8 [E][24], waypoints double [E][64][3], nwp int32 [E] (synchronises) */
int bp_bd_get_state(bp_handle *h, uint8_t *alive, double *waypoints, int32_t *nwp);

/* ---- rgb_array frames (benchpush/common/utils/renderer.py Renderer.render; benchpush_amd/render.py states the frame) ----
 * A frame is uint8 [H][W][3], row 0 at the top.  World point (x, y) maps to the frame point
 *   col = (x + tx) * scale + cx,   row = cy - (y + ty) * scale     (binary64, in this order)
 * and pixel (r, c) is sampled at the point (col c, row r).  A polygon (3+ vertices) covers the pixels that skimage's point_in_polygon
 * rule accepts; a capsule (segment a-b, half-width h) covers the pixels with dist2 <= h*h.  Painter's order, bottom first: the background,
 * the primitives of layer 0, the shape slots in the table's order, the path segments of the frame's env, the primitives of layer 1. */
#define BP_RENDER_MAX_PRIMS 256
#define BP_RENDER_PRIM_VERTS 8
#define BP_RENDER_MAX_SIDE 8192            /* frame width and height cap */
#define BP_RENDER_MAX_PIXELS (1 << 24)     /* frame area cap (W * H) */
#define BP_RENDER_MAX_PATH 4096            /* path points per env */
typedef struct bp_render_prim {
    int32_t kind;     /* 0: filled polygon of nv (3..8) world vertices; 1: capsule from v[0] to v[1] */
    int32_t layer;    /* 0: under the shapes (box-delivery receptacle); 1: over the shapes and the paths (goal line, goal disc, clearance boundary) */
    uint32_t rgb;     /* r | g << 8 | b << 16 */
    int32_t nv;
    double half_px;   /* capsule half-width = half_px + half_world * scale */
    double half_world;
    double v[BP_RENDER_PRIM_VERTS][2];
} bp_render_prim;
typedef struct bp_render_args {
    double scale, tx, ty, cx, cy;    /* the transform above */
    int32_t width, height;           /* frame size in pixels */
    uint32_t background;             /* r | g << 8 | b << 16 */
    int32_t max_path;                /* path points per env in `paths` (0: no paths) */
    double path_half_px;             /* half-width of the path segments, in pixels */
} bp_render_args;
int32_t bp_sizeof_render_args(void);
int32_t bp_sizeof_render_prim(void);
/* Per-slot draw table, host buffers, copied at call time.  order int32 [T][nslot]: the slots of trial t bottom first, -1 = none (slots at or
 * above the env's body count are skipped too); rgb uint32 [T][nslot] colour of slot s in trial t; prims [nprim] (nprim <= BP_RENDER_MAX_PRIMS).
 * T must equal the handle's trial count and nslot its slot capacity (bp_nb_cap).  Slots with 2 vertices (maze walls) are capsules of
 * half-width shape radius * scale; polygons ignore the shape radius.  Box-delivery / area-clearing: removed boxes are not drawn. */
int bp_set_render_table(bp_handle *h, int32_t T, int32_t nslot, const int32_t *order, const uint32_t *rgb, int32_t nprim, const bp_render_prim *prims);
/* k frames of the envs env_ids[0..k) (device int32 [k]) into out (device uint8 [k][H][W][3]; 64-bit offsets).  paths: device double
 * [k][max_path][2] world points and path_len device int32 [k] (points used, clamped to max_path), or both null.  Reads the handle's state
 * only and runs on `stream` after the work already queued there (a step's forked work joins back to the caller's stream).  BP_EINVAL for
 * ids outside [0, E), k <= 0, scale <= 0 or a frame above the caps; BP_ESTATE before bp_set_render_table or bp_reset.  Synchronises
 * `stream` once to check the ids. */
int bp_render(bp_handle *h, const bp_render_args *args, const int32_t *env_ids, int32_t k, const double *paths, const int32_t *path_len,
              uint8_t *out, void *stream);

/* ---- saving, restoring and forking environments (state records) ----
 * Between two steps an env is a fixed-size byte image, the state record: a 32-byte header (magic, record size, 64-bit layout id, 8 reserved bytes) and one
 * segment per persistent per-env array (body state, the 64 arbiter slots, the per-env scalars, the last step's reward / flags, the episode metrics;
 * box-delivery / area-clearing: box bookkeeping, waypoints and the robot's distance map), every segment on a 16-byte boundary.  Left out: dispatch-order
 * hints, scheduler queues, timers and cumulative counters of the handle -- results never depend on them.  The layout id hashes the env kind and task, the
 * capacities (body slots, BP_MAXV, neighbour and arbiter slots, box and waypoint slots, map cells), the bytes of the handle's configuration struct (padding
 * included: zero it) and the scenario tables as uploaded by the loader; the number of envs and env_id_offset are NOT part of it, so a record may be loaded
 * into any handle created with the same configuration and the same trials.  Records do not survive another configuration, other trials or another library build.
 *   env_ids / src_ids / dst_ids  device int32 [k], ids in [0, E) (the reset templates are not addressable)
 *   records                      device uint8 [k][record bytes], 16-byte aligned
 * All work is enqueued on `stream` after the work already queued there.  BP_ESTATE before the first reset.  With flags == 0 the calls synchronise `stream`
 * once to check their arguments on the host and return BP_EINVAL WITHOUT touching any env for: an id outside [0, E), a destination named twice, (clone) a
 * destination that is also a source, (load) a header with a wrong magic, size or layout id.  Saving always checks its ids.  BP_STATE_TRUSTED skips checks and
 * synchronisation (planners that call this in a loop); what an unchecked bad argument does is undefined.  A source may be repeated (fan-out 1 -> n).
 * A restored env continues exactly (bit for bit) as the saved one would have until its episode ends; per-env error bits saved in a record are OR-ed into the
 * destination's, never cleared.  At its next reset the DESTINATION env draws its trial and its random_start pose from its OWN global id and the restored
 * episode counter: trial (env_id_offset + env + episode) % T, like every other reset of that env. */
#define BP_STATE_TRUSTED 1
int64_t bp_state_bytes(const bp_handle *h);          /* bytes of one record; < 0 before the scenarios are loaded */
uint64_t bp_state_layout_id(const bp_handle *h);     /* 0 before the scenarios are loaded */
int bp_save_state(bp_handle *h, const int32_t *env_ids, int32_t k, uint8_t *records, void *stream);
int bp_load_state(bp_handle *h, const int32_t *env_ids, int32_t k, const uint8_t *records, int32_t flags, void *stream);
int bp_clone_state(bp_handle *h, const int32_t *src_ids, const int32_t *dst_ids, int32_t k, int32_t flags, void *stream);
/* The record layout as a pure function (no GPU, no handle): env_kind BP_ENV_*, task (box handles: 0 box-delivery, 1 area-clearing), nbcap body slots
 * (a multiple of 8), map_cells = cells of a box handle's small-map window (0 otherwise).  Returns the number of segments (the header is segment 0) or a negative
 * BP_E*; writes the first max_segments rows of offsets_host / bytes_host (int64: offset in the record, bytes per env) and widths_host (int32: widest access
 * in bytes), the record size and the part of the layout id that these shapes decide.  Any pointer may be NULL. */
int bp_state_layout_query(int32_t env_kind, int32_t task, int32_t nbcap, int32_t map_cells, int32_t max_segments, int64_t *offsets_host,
                          int64_t *bytes_host, int32_t *widths_host, int64_t *total_bytes, uint64_t *structure_id);

/* ---- swath costs of candidate paths over the cost maps ----
 * compute_swath_cost of the reference (common/swath.py:114-163; the sum inside AStar.get_swath_cost and Path.update) for K candidate paths of every env in
 * one launch (DESIGN.md "Swath costs" states the semantics exactly).  All arrays are device memory:
 *   cost_maps  double [E][H][W] with map_stride doubles between the envs' maps, or one [H][W] map for all envs with map_stride 0
 *   paths      double [E][K][P][3]: samples (x, y, theta) in cost-map cells / radians
 *   lengths    int32 [E][K] or NULL (all P): samples that count, clamped to [0, P] on the device
 *   rows       int32 [E][K][2] or NULL (all rows): the swath is restricted to rows lo <= r < hi, each bound clamped to [0, H] on the device
 *   footprint  double [nv][2] in cells, 3 <= nv <= BP_MAXV (20), any simple polygon
 *   costs      double [E][K]
 *   swaths     uint8 [E][K][H][W] (0 / 1, row window applied) or NULL
 * A pixel (row r, column q) is covered by a sample iff skimage's point_in_polygon holds for (x = q, y = r) and the vertices
 * (x + (c*vx - s*vy), y + (s*vx + c*vy)), (s, c) the library's deterministic sin / cos of theta; a candidate's swath is the union over its counted
 * samples.  The cost adds the map's covered cells per row in ascending column order and the row sums in ascending row order, each from +0.0.
 * BP_SWATH_CLIP ignores what lies off the map; BP_SWATH_REJECT gives +inf if any transformed vertex of a counted sample lies outside
 * [0, W-1] x [0, H-1] (the mask is still the clipped one).  A non-finite component in a counted sample: NaN, empty mask.  A finite sample with |x|, |y|
 * or |theta| above 1e15 counts as off the map as a whole.
 * The bit image of the swath lives in LDS: H * ceil(W / 64) <= 4096 is required (380 x 60: 380).  BP_EINVAL, with nothing launched or written, for a
 * NULL required pointer, H, W, K, P <= 0, nv outside [3, 20], a grid above that limit, an unknown mode, 0 < map_stride < H * W or a handle that is
 * not ship-ice; BP_ESTATE before load and reset.  Reads the handle's device only: no environment state is touched.  Enqueued on `stream`. */
#define BP_SWATH_CLIP 0
#define BP_SWATH_REJECT 1
typedef struct bp_swath_config {
    int32_t H, W;           /* rows and columns of a cost map */
    int32_t K, P;           /* candidates per env, samples per candidate */
    int32_t nv;             /* footprint vertices */
    int32_t outside;        /* BP_SWATH_CLIP / BP_SWATH_REJECT */
    int64_t map_stride;     /* doubles between the envs' maps; 0: one map shared by all */
} bp_swath_config;
int32_t bp_sizeof_swath_config(void);
int bp_swath_cost(bp_handle *h, const bp_swath_config *cfg, const double *cost_maps, const double *paths, const int32_t *lengths, const int32_t *rows,
                  const double *footprint, double *costs, uint8_t *swaths, void *stream);

/* ---- batched lattice A* over the cost maps ----
 * AStar.search of the reference (baselines/ship_ice_nav/planning_based/utils/a_star_search.py; high-level planner: goal line, no occupancy model, no
 * smoothing) for every env in one launch, one wavefront per env (DESIGN.md "Lattice search" states the semantics exactly; tests/lattice_ref.py restates
 * them).  Device memory:
 *   cost_maps  double [E][H][W] with map_stride doubles between the envs' maps, or one [H][W] map with map_stride 0
 *   starts     double [E][3] = (x, y, theta) in cells / radians;  goal_y double [E] in cells
 *   active     uint8 [E] or NULL: envs with 0 are BP_LATTICE_SKIPPED; only their status is written
 *   masks      uint64 [E or 1][nh * ne_max][S]: word r of key (h * ne_max + k) is row r of the S x S swath mask of edge k taken from a node of
 *              heading h (bit c = column c), the node at the centre cell; mask_stride words between the envs' tables, 0 for one shared table
 *   workspace  bp_lattice_workspace_bytes(cfg, E) bytes, 16-byte aligned; contents need not be kept between calls
 *   status int32 [E]; g double [E] (+inf unless found); expanded int32 [E]; n_nodes int32 [E] (0 unless found);
 *   nodes double [E][max_path_nodes][3] = (X, Y, world heading) start to goal and edges int32 [E][max_path_nodes] = base * ne_max + k of the edge that led
 *   to each node, -1 for the start: rows 0 .. n_nodes-1 of found envs are written, nothing else
 * Host memory (copied into the launch): per base heading b < nb = nh / 4 the edges double [nb][ne_max][2] in lattice units, their headings
 * int32 [nb][ne_max], their path lengths double [nb][ne_max] in cells and the edge counts int32 [nb].
 * BP_EINVAL, with nothing launched or written, for: a handle that is not ship-ice, S > 64 or even, nh not 8 / 16 or nb != nh / 4, more than 32 edges per
 * base heading, an edge that is not a multiple of unit / den or an edge heading outside [0, nh), non-positive sizes or caps, a map whose diagonal exceeds
 * 4094 sub-units, bad strides, a workspace that is too small or misaligned.  BP_ESTATE before load and reset.  Reads no environment state. */
enum { BP_LATTICE_FOUND = 0, BP_LATTICE_NO_PATH = 1, BP_LATTICE_CAP = 2, BP_LATTICE_SKIPPED = 3 };
typedef struct bp_lattice_config {
    int32_t H, W;               /* rows and columns of a cost map */
    int32_t S;                  /* mask side = 2 * max_val + 1 <= 64 */
    int32_t nh, nb;             /* headings (8 or 16), base headings (nh / 4) */
    int32_t ne_max;             /* second dimension of the edge tables and of the mask keys, <= 32 */
    int32_t den;                /* sub-units per lattice unit (2 for the reference's 8-heading set: its (1.5, 1.5, 1) edge) */
    int32_t margin;             /* row window: [max(0, int(y0) - margin), min(H, int(goal_y) + margin)) */
    int32_t h_baseline;         /* != 0: h = max(0, goal_y - Y) instead of the Dubins heuristic */
    int32_t max_expansions, node_capacity, queue_capacity, max_path_nodes;   /* caps: exceeding one gives BP_LATTICE_CAP */
    int32_t pad_;
    int64_t map_stride, mask_stride;
    double unit;                /* cells per lattice unit (the primitives' scale) */
    double weight;              /* f = g + weight * h; 0: f = g */
    double turning_radius;      /* cells */
} bp_lattice_config;
int32_t bp_sizeof_lattice_config(void);
int64_t bp_lattice_workspace_bytes(const bp_lattice_config *cfg, int32_t num_envs);   /* < 0: BP_EINVAL */
int bp_lattice_search(bp_handle *h, const bp_lattice_config *cfg, const double *cost_maps, const double *starts, const double *goal_y, const uint8_t *active,
                      const double *edges_host, const int32_t *edge_headings_host, const double *edge_lengths_host, const int32_t *edge_counts_host,
                      const uint64_t *masks, void *workspace, int64_t workspace_bytes, int32_t *status, double *g, int32_t *expanded, int32_t *n_nodes,
                      double *nodes, int32_t *edges, void *stream);

/* ---- tracking planned paths ----
 * The controller of the reference's planning-based policy (PlanningBasedPolicy.act, baselines/ship_ice_nav/planning_based/policy.py:61-172) for every
 * env in one launch, one wavefront per env (DESIGN.md "Path tracking" states the semantics exactly; tests/track_ref.py restates them).  Device memory:
 *   paths    double [E][P][3]: samples (x, y, theta) with path_stride doubles between the envs' paths, or one [P][3] path for all envs with path_stride 0
 *   lengths  int32 [E] or NULL (all P): samples that count, at most P
 *   poses    double [E][3] = (x, y, yaw) of the ship, in the units of the paths
 *   active   uint8 [E] or NULL (all)
 *   state    double [E][4] = (int_yaw, prev_yaw, int_v, has_yaw): the integrators that the controller keeps between calls, read and written; has_yaw is
 *            0.0 until the PID branch has run once (the reference's hasattr test), then 1.0.  A zeroed row is a fresh controller.
 *   actions  double [E][2] = (omega / action_scale, 20 * v_cmd): the yaw action of bp_step and the surge command
 *   ct_err   double [E]: distance to the nearest counted sample
 *   diag     int32 [E][4] or NULL = (i_near, branch, forward index, backward index); branch BP_TRACK_NONE 0, BP_TRACK_GENTLE 1 (fixed-rate turn),
 *            BP_TRACK_PID 2, BP_TRACK_NEAR 3.  The forward index is the carrot's in branches 1 and 2 and the end of the slice ahead in branch 3.
 * An env with active == 0 or a length below 1 has nothing written, its state row included.  A non-finite component in the pose or in a counted sample:
 * NaN actions and ct_err, diag (-1, 0, -1, -1), the state row untouched.
 * BP_EINVAL, with nothing launched or written, for a NULL required pointer, P <= 0, 0 < path_stride < 3 * P or a negative one, dt or action_scale that
 * is not positive and finite, or a handle that is not ship-ice; BP_ESTATE before load and reset.  Reads the handle's device and size only: no environment
 * state is touched.  Enqueued on `stream`; a function of its inputs bit for bit. */
enum { BP_TRACK_NONE = 0, BP_TRACK_GENTLE = 1, BP_TRACK_PID = 2, BP_TRACK_NEAR = 3 };
typedef struct bp_track_config {
    int32_t P;                                      /* samples per path */
    int32_t pad_;
    double thresh, look_car, d_back, d_ahead;       /* cross-track switch (10); carrot distance when far (50); slice behind (15) and ahead (25) */
    double kp, ki, kd, i_cap, dead;                 /* yaw-rate PID: 0.10, 0.15, 2.0; integrator cap 10; dead zone 0.02 */
    double straight_ang, yaw_big, omega_small;      /* straight-slice turn: 0.100, 0.50, 0.002 */
    double kp_v, ki_v, v_max, omega_max;            /* surge PI: 0.50, 0.05, 2.5; yaw-rate cap 0.02 */
    double dt;                                      /* 0.005 */
    double action_scale;                            /* the env's max_yaw_rate_step */
} bp_track_config;
int32_t bp_sizeof_track_config(void);
int bp_track_path(bp_handle *h, const bp_track_config *cfg, const double *paths, int64_t path_stride, const int32_t *lengths, const double *poses,
                  const uint8_t *active, double *state, double *actions, double *ct_err, int32_t *diag, void *stream);

/* ---- batched RRT and the waypoint controller (maze handles) ----
 * bp_rrt_plan: the reference's two-pass RRT (baselines/maze_NAMO/planning_based/RRT/rrt.py: RRTPlanner.plan, _run_rrt) followed by _densify and the
 * policy's prune_by_distance, for every env in one launch, one wavefront per env (DESIGN.md "RRT" states the semantics and where they deviate from
 * the reference; tests/rrt_ref.py restates them and the kernel is held to == against it).  Device memory, contiguous:
 *   starts, goals  double [E][2]
 *   walls          double [n_walls][4] = (ax, ay, bx, by), shared by all envs; n_walls <= BP_RRT_MAX_WALLS (may be 0, then walls may be NULL)
 *   boxes          double [E][n_boxes][n_verts][2] with counts int32 [E][n_boxes]: convex polygons of 3 .. n_verts vertices, either winding; a count of
 *                  0 skips the polygon; n_verts <= BP_MAXV and n_boxes * n_verts <= BP_RRT_MAX_BOX_VERTS (n_boxes may be 0, then both may be NULL)
 *   streams        int64 [E]: the env's RNG stream.  A plan is a function of the config, the env's own inputs and its stream only -- not of E or of
 *                  the env's place in the batch.  Sample j of iteration k of pass p is bp_rrt_uniform(seed, stream, p, k, j).
 *   active         uint8 [E] or NULL (all)
 *   workspace      bp_rrt_workspace_bytes(cfg, E) bytes, 16-byte aligned: per env (max_nodes + 2) nodes as (x, y) doubles, then (max_nodes + 2)
 *                  int32 parents, rounded up to 16 bytes -- 520 KB per env at the reference's max_nodes of 26000, 2.1 GB for 4096 envs.  Inactive
 *                  envs still own their slice; a caller short of memory plans a group of envs per call through `active` with a handle of that size.
 *                  After the call an env's slice holds the tree of the last pass it ran (nodes 0 .. n_nodes - 1 and their parents, -1 at node 0).
 *   status         int32 [E], BP_RRT_*
 *   n_nodes, iterations  int32 [E][2]: per pass, the tree's size (the goal node included when found) and the loop iterations used; 0 for a pass not run
 *   paths          double [E][max_waypoints][2] and lengths int32 [E]: the pruned waypoints; rows from `lengths` on are not written
 * Status: BP_RRT_FOUND (pass 0, boxes block) and BP_RRT_FOUND_IGNORING_BOXES (pass 1): the pruned waypoints.  BP_RRT_FALLBACK (every pass used up
 * max_nodes) and BP_RRT_BLOCKED (start or goal within inflate_radius of a wall; no search): the path [start, goal], as the reference returns.
 * BP_RRT_CAP (more than max_waypoints waypoints): length 0, the first max_waypoints waypoints are in `paths`.  BP_RRT_BAD_INPUT (a non-finite start,
 * goal, wall or counted vertex, or a count outside 0, 3 .. n_verts): length 0.  BP_RRT_SKIPPED (active == 0): nothing but the status is written.
 * BP_EINVAL, with nothing launched or written, for a NULL required pointer, a handle that is not a maze, step <= 0, goal_radius < 0, max_nodes < 1,
 * max_waypoints < 2, passes outside 1 .. 2, a non-finite or negative config value, more than 2^22 dense points in all
 * ((max_nodes + 2) * max(1, max(step, goal_radius) / max(1e-3, densify_ds)): what bounds _densify), sizes over the caps above, or a workspace that is short or not 16-byte aligned; BP_ESTATE before
 * load and reset.  Reads the handle's device and size only.  Enqueued on `stream`; a function of its inputs bit for bit.
 * BP_RRT_LDS_NODES in the environment (read at every call; a multiple of 64 up to 2048, 0: none) is how many of the tree's first nodes the nearest
 * search keeps in LDS; it changes the time of a launch and nothing else (profiles/rrt/README.md). */
#define BP_RRT_MAX_WALLS 128
#define BP_RRT_MAX_BOX_VERTS 1280
enum { BP_RRT_FOUND = 0, BP_RRT_FOUND_IGNORING_BOXES = 1, BP_RRT_FALLBACK = 2, BP_RRT_BLOCKED = 3, BP_RRT_CAP = 4, BP_RRT_BAD_INPUT = 5, BP_RRT_SKIPPED = 6 };
typedef struct bp_rrt_config {
    double step, goal_radius, goal_bias;   /* rrt_config.yaml: 0.05, 0.01, 0.01 */
    double densify_ds, prune_min_dist;     /* 0.08; policy.py's prune_by_distance(min_dist=0.3) */
    double inflate_radius;                 /* walls block within this distance: the reference's 1.5 * (1.5 * robot.min_r) */
    uint64_t seed;                         /* 42 */
    int32_t max_nodes;                     /* iterations per pass: 26000 */
    int32_t max_waypoints;                 /* rows of `paths` per env */
    int32_t passes;                        /* 2; 1: boxes always block, no second pass */
    int32_t pad_;
} bp_rrt_config;
int32_t bp_sizeof_rrt_config(void);
int64_t bp_rrt_workspace_bytes(const bp_rrt_config *cfg, int32_t num_envs);   /* BP_EINVAL (negative) for a config that bp_rrt_plan refuses */
double bp_rrt_uniform(uint64_t seed, int64_t stream, int32_t pass, int32_t iteration, int32_t draw);   /* host function; the kernel's draws */
int bp_rrt_plan(bp_handle *h, const bp_rrt_config *cfg, const double *starts, const double *goals, const double *walls, int32_t n_walls,
                const double *boxes, const int32_t *counts, int32_t n_boxes, int32_t n_verts, const int64_t *streams, const uint8_t *active,
                void *workspace, int64_t workspace_bytes, int32_t *status, int32_t *n_nodes, int32_t *iterations, double *paths, int32_t *lengths,
                void *stream);

/* bp_track_waypoints: what the reference's maze policy does with the path at every step (policy.py: act builds a fresh DP and calls
 * DP.ideal_control, common/controller/dp.py), so the controller keeps no state: the nearest waypoint (first minimum), advanced while it is within Lfc
 * and a next one exists; theta_e = atan2(sin(e), cos(e)), e = atan2(yd - y, xd - x) - yaw; action = theta_e / dt / action_scale.
 *   paths double [E][P][2], lengths int32 [E] or NULL (all P), poses double [E][3] = (x, y, yaw), active uint8 [E] or NULL,
 *   actions double [E], diag int32 [E][2] = (nearest index, target index)
 * An env with active == 0, a length below 1, or a non-finite pose or counted waypoint gets a NaN action and diag (-1, -1).  BP_EINVAL, with nothing
 * launched, for a NULL required pointer, P <= 0, Lfc that is not finite, dt or action_scale that is not positive and finite, or a handle that is not
 * a maze; BP_ESTATE before load and reset. */
typedef struct bp_track_wp_config {
    int32_t P;                /* waypoints per path */
    int32_t pad_;
    double Lfc, dt;           /* rrt_config.yaml controller: look-ahead 0.5, dt 0.8 */
    double action_scale;      /* the env's max_yaw_rate_step */
} bp_track_wp_config;
int32_t bp_sizeof_track_wp_config(void);
int bp_track_waypoints(bp_handle *h, const bp_track_wp_config *cfg, const double *paths, const int32_t *lengths, const double *poses,
                       const uint8_t *active, double *actions, int32_t *diag, void *stream);

/* ---- the GTSP push planner and its controller (area-clearing handles) ----
 * bp_gtsp_plan: the reference's planning-based area-clearing baseline (baselines/area_clearing/planning_based/policy.py: plan_path;
 * GTSPPlanner/transition_graph_lookup.py; create_instance.py) for every env in one launch, one wavefront per env, with an exact set DP in the place of
 * the GLNS heuristic (DESIGN.md "GTSP" states the semantics and the deviations; tests/gtsp_ref.py restates them and the kernels are held to ==
 * against it).  A box is pushed iff it intersects the handle's clearance boundary; cluster c is the c-th pushed box in slot order, node c * G + g
 * pushes it to goal segment g, the robot is node n * G.  Device memory, contiguous:
 *   poses          double [E][3] = (x, y, theta)
 *   boxes          double [E][n_boxes][n_verts][2] with counts int32 [E][n_boxes]: convex polygons of 3 .. n_verts vertices, either winding; a count
 *                  of 0 skips the slot; n_boxes <= BP_GTSP_MAX_SLOTS, n_verts <= BP_MAXV
 *   goals          double [num_goals][4] = (ax, ay, bx, by), shared by all envs
 *   active         uint8 [E] or NULL (all)
 *   workspace      bp_gtsp_workspace_bytes(cfg, E) bytes, 16-byte aligned: per env the DP table int32 [2^max_boxes][max_boxes * num_goals]
 *                  (160 KB at 10 boxes and 4 goals, 1.5 MB at the caps)
 *   status         int32 [E]: BP_GTSP_* in the low byte, BP_GTSP_FLAG_* above it
 *   n_push, cost, lengths  int32 [E]: pushed boxes, the tour's integer cost (robot -> nodes -> robot), rows of the path (2 * n_push + 1)
 *   tour           int32 [E][max_boxes]: node indices in visiting order; entries from n_push on are not written
 *   paths          double [E][2 * max_boxes + 1][3]: the pose, then per visited node (route start, heading) and (route end, heading)
 *   track_id, track_setpoint  int32 [E], double [E][2]: the controller's first state (1, TargetCourse.init_setpoint on the path)
 *   weights        int32 [E][N_max][N_max] or NULL, N_max = max_boxes * num_goals + 1: the matrix, its N x N block written (N = n_push * num_goals + 1)
 * Status: BP_GTSP_OK; BP_GTSP_NOTHING_TO_PUSH (the path is the pose alone); BP_GTSP_SKIPPED (active == 0: nothing but the status is written);
 * BP_GTSP_CAP (more than max_boxes boxes to push: n_push is written, length 0); BP_GTSP_INVALID (a non-finite pose, goal or counted vertex, or a
 * count outside 0, 3 .. n_verts: length 0).  BP_GTSP_FLAG_VANISHED: a box to push left nothing when shrunk and was skipped;
 * BP_GTSP_FLAG_DEGENERATE: a shrunk box touched a goal segment, its route is one point.
 * BP_EINVAL, with nothing launched or written, for a NULL required pointer, a handle that is not area-clearing, max_boxes outside
 * 1 .. BP_GTSP_MAX_BOXES, num_goals outside 1 .. BP_GTSP_MAX_GOALS, round_decimals outside 0 .. 15, a negative or non-finite length, speed or scale,
 * sizes over the caps above, or a workspace that is short or not 16-byte aligned; BP_ESTATE before load and reset.  Reads the handle's device, size
 * and boundary only.  Enqueued on `stream`; a function of its inputs bit for bit.
 *
 * bp_gtsp_track: PlanningBasedPolicy.act after planning.  Per env: past the path's end the action is (0, 0); within switch_dist of waypoint
 * track_id the id advances (past the end: (0, 0)) and the setpoint becomes that waypoint; then DP.ideal_control: omega = wrap(atan2(yd - y, xd - x)
 * - yaw) / dt, speed = |R(yaw) (target_speed, 0)|.  actions double [E][2] = (speed / v_scale, omega / w_scale), diag int32 [E] = the id.  An env with
 * active == 0, a length below 2, a negative id or a non-finite pose or counted waypoint gets NaN actions and diag -1, and its state is left as it is. */
#define BP_GTSP_MAX_BOXES 12
#define BP_GTSP_MAX_GOALS 8
#define BP_GTSP_MAX_SLOTS 64
enum { BP_GTSP_OK = 0, BP_GTSP_NOTHING_TO_PUSH = 1, BP_GTSP_SKIPPED = 2, BP_GTSP_CAP = 3, BP_GTSP_INVALID = 4,
       BP_GTSP_FLAG_VANISHED = 0x100, BP_GTSP_FLAG_DEGENERATE = 0x200 };
typedef struct bp_gtsp_config {
    double shrink, extend;             /* policy.py: buffer(-0.4), EXTEND_BUFFER = 2 */
    double lin_vel, ang_vel;           /* transition_graph_lookup.py: 0.5, pi / 4 */
    double Lfc, dt, target_speed;      /* gtsp_config.yaml controller: 0.5, 0.8, 0.2 */
    double switch_dist;                /* policy.py act: 0.4 */
    double v_scale, w_scale;           /* the env's target_speed and max_yaw_rate_step */
    int32_t round_decimals;            /* np.round(.., 7) */
    int32_t max_boxes, num_goals;
    int32_t pad_;
} bp_gtsp_config;
int32_t bp_sizeof_gtsp_config(void);
int64_t bp_gtsp_workspace_bytes(const bp_gtsp_config *cfg, int32_t num_envs);   /* BP_EINVAL (negative) for a config that bp_gtsp_plan refuses */
int bp_gtsp_plan(bp_handle *h, const bp_gtsp_config *cfg, const double *poses, const double *boxes, const int32_t *counts, int32_t n_boxes,
                 int32_t n_verts, const double *goals, const uint8_t *active, void *workspace, int64_t workspace_bytes, int32_t *status,
                 int32_t *n_push, int32_t *tour, int32_t *cost, double *paths, int32_t *lengths, int32_t *track_id, double *track_setpoint,
                 int32_t *weights, void *stream);
int bp_gtsp_track(bp_handle *h, const bp_gtsp_config *cfg, const double *paths, const int32_t *lengths, const double *poses, const uint8_t *active,
                  int32_t *track_id, double *track_setpoint, double *actions, int32_t *diag, void *stream);

/* ---- replay buffer on the ready queue (DESIGN.md "Replay buffer") ----
 * Handle-free: the caller owns every array (device memory on `device`) and passes them in a bp_replay_desc.  C = capacity, E = num_envs, R = row_bytes
 * (P * P * 4, a multiple of 16; every observation array 16-byte aligned).
 *   ring     state, next_state uint8 [C][R]; action int32 [C]; reward, ministeps float [C]; nonfinal uint8 [C]; env int32 [C]
 *   per env  pend_obs uint8 [E][R]; pend_action int32 [E]; pend_flags uint8 [E]: bit 0 an observation is held, bit 1 an action is recorded,
 *            bit 2 the env awaits a record
 *   hdr      int64 [4]: transitions ever stored, sample draws made, transition rows dropped for want of a pending observation or action, rejected record rows
 *   workspace row_slot int32 [max_rows], win int32 [E] (contents are scratch)
 * All of it starts as zeros.
 *
 * bp_replay_observe takes the outputs of one bp_bd_queue_recv (M <= max_rows rows; info is [M][BP_INFO_COUNT], ministeps_col its column of info['ministeps']).
 * Rows with ids[j] = e in [0, E) are handled in ascending j (other rows are ignored).  A row is a transition row if slices[j] > 0 and bits 0 and 1 of e are
 * set; it is stored at slot (hdr[0] + rank) % C, rank its rank among the call's transition rows: state = pend_obs[e], next_state = obs[j], action =
 * pend_action[e], reward = (float)reward[j], ministeps = (float)info[j][ministeps_col], nonfinal = !terminated[j] (the reference builds no next observation
 * for a terminated step; truncated is accepted and not read), env = e.  A row with slices[j] > 0 that lacks a bit stores nothing and counts in hdr[2].
 * Then every handled row, fresh rows (slices 0) included, makes obs[j] the pending observation of e and sets its flags to bit 0 | bit 2.  hdr[0] grows by
 * the number of transition rows; if more than C arrive in one call the later ones overwrite the earlier ones in row order.  The ids of one call must be
 * distinct, as the queue's are.
 *
 * bp_replay_record takes what is passed to bp_bd_queue_send (action_dim 1; reset [M] or NULL).  Row j is accepted if ids[j] = e in [0, E), bit 2 of e is set
 * and j is the smallest row naming e.  Accepted without reset: pend_action[e] = (int)actions[j], bit 1 set, bit 2 cleared; accepted with reset[j] != 0: all
 * bits cleared.  Every other row with ids[j] >= 0 counts in hdr[3].
 *
 * bp_replay_sample draws B transitions with replacement: n = min(hdr[0], C) on the device, sample b takes slot bp_replay_index(seed, hdr[1], b, n), then
 * hdr[1] grows by one.  out: state, next_state float [B][4][P][P] (channel first, (float)u8 / 255.0f by IEEE division), action int64 [B], reward, ministeps
 * float [B], nonfinal uint8 [B], slot int32 [B], valid uint8 [B] = 1 when n > 0; with n == 0 every output is zero.  The float planes are 16-byte aligned.
 * bp_replay_index is a host function, the kernel's index rule: the high 32 bits r of the project's counter RNG keyed by (seed, draw, b), (r * n) >> 32;
 * -1 for n outside 1 .. 2^31 - 1.
 *
 * Nothing synchronises, nothing is read back; all work is enqueued on `stream`.  BP_EINVAL, before anything is launched: a NULL pointer, row_bytes % 16 != 0,
 * capacity < 1, num_envs < 1, action_dim != 1, M or B < 1, M > max_rows, ministeps_col outside the info row.  (Added within ABI 11: the additions only add.) */
typedef struct bp_replay_desc {
    int32_t capacity, num_envs, device, action_dim;
    int64_t row_bytes;
    int32_t max_rows, pad_;
    uint8_t *state, *next_state;
    int32_t *action;
    float *reward, *ministeps;
    uint8_t *nonfinal;
    int32_t *env;
    uint8_t *pend_obs;
    int32_t *pend_action;
    uint8_t *pend_flags;
    int64_t *hdr;
    int32_t *row_slot, *win;
} bp_replay_desc;
typedef struct bp_replay_batch {
    float *state, *next_state;
    int64_t *action;
    float *reward, *ministeps;
    uint8_t *nonfinal;
    int32_t *slot;
    uint8_t *valid;
} bp_replay_batch;
int32_t bp_sizeof_replay_desc(void);
int32_t bp_sizeof_replay_batch(void);
int64_t bp_replay_index(uint64_t seed, int64_t draw, int32_t b, int64_t n);
int bp_replay_observe(const bp_replay_desc *d, const int32_t *ids, const uint8_t *obs, const double *reward, const uint8_t *terminated,
                      const uint8_t *truncated, const double *info, const int32_t *slices, int32_t M, int32_t ministeps_col, void *stream);
int bp_replay_record(const bp_replay_desc *d, const double *actions, const int32_t *ids, const uint8_t *reset, int32_t M, void *stream);
int bp_replay_sample(const bp_replay_desc *d, int32_t B, uint64_t seed, const bp_replay_batch *out, void *stream);

/* ---- on-policy rollout buffer with GAE (DESIGN.md "Rollout buffer") ----
 * Handle-free: the caller owns every array (device memory on `device`) and passes them in a bp_rollout_desc.  T = n_steps, E = num_envs, A = action_dim,
 * R = row_bytes (a multiple of 16; the rows are uint8 and their shape is opaque to the library; every observation array is 16-byte aligned), N = T * E
 * (at most 2^31 - 1).
 *   obs uint8 [T][E][R]; action float [T][E][A]; reward, value, logp, advantage, ret float [T][E]; episode_start uint8 [T][E]; last_done uint8 [E]
 *   hdr int64 [2]: hdr[0] truncated rows left without a bootstrap, hdr[1] rows stored (E per bp_rollout_end)
 * All of it starts as zeros.  The step index t, the epoch and the minibatch number are host integers: the call sequence does not depend on data.
 *
 * bp_rollout_begin, before the env step: obs[t] = the [E][R] batch the policy acted on (the env rewrites its buffer in place), action[t], value[t],
 * logp[t] = the float [E][A] / [E] / [E] arguments, episode_start[t] = last_done.
 *
 * bp_rollout_pick_rows: the first K envs in ascending order with mask[e] != 0: out_ids[k] = e and out_rows[k] = (float)src[e][.] / 255.0f as float [K][R]
 * (an IEEE division, not a reciprocal); rows beyond the number found get out_ids = -1 and zeros; hdr[0] += the number of masked envs beyond K.  This is the
 * fixed-size batch on which the policy evaluates V(terminal observation) of the truncated envs without a host read.  src uint8 [E][R], out_rows 16-byte aligned.
 *
 * bp_rollout_end, after the env step: reward[t][e] = (float)reward[e] (reward is double [E]); then for every k < K with boot_ids[k] = e in [0, E):
 * reward[t][e] = reward[t][e] + (float)gamma * boot_values[k] (the ids >= 0 of one call must be distinct, as bp_rollout_pick_rows makes them; boot_ids may
 * be NULL, K is then not read); last_done = done (uint8 [E]); hdr[1] += E.
 *
 * bp_rollout_finish, the GAE scan backwards over t, all in float, in exactly this order (g = (float)gamma; gl = (float)gl, the caller computes
 * (double)gamma * (double)lambda): nn = 1 - done_next; delta = (reward[t] + (g * v_next) * nn) - value[t]; adv = delta + (gl * nn) * adv;
 * advantage[t] = adv; ret[t] = adv + value[t].  For t = T - 1, v_next and done_next are last_values (float [E]) and last_done, otherwise value[t + 1] and
 * episode_start[t + 1]; adv starts at 0.
 *
 * bp_rollout_minibatch: sample b of minibatch j takes the flat index i = bp_rollout_index(seed, epoch, j * B + b, N), t = i / E, e = i % E, and writes
 * out->obs float [B][R] ((float)u8 / 255.0f by IEEE division, 16-byte aligned), action float [B][A], value, logp, advantage, ret float [B], index int32 [B],
 * valid uint8 [B]; samples with j * B + b >= N have valid = 0 and zeros everywhere.  j * B < N.
 *
 * bp_rollout_index is a host function, the kernel's rule: a keyed bijection of [0, N), so an epoch visits every stored transition exactly once.  It is a
 * 4-round balanced Feistel network over 2h bits, h the smallest value with 4^h >= N: x = i; (left, right) = (x >> h, x & (2^h - 1)); round r = 0 .. 3 maps
 * (left, right) to (right, left ^ F) with F = the low h bits of S[key ^ (r << 32 | right)] >> 32, key = S[seed ^ S[epoch]], S the splitmix64 step of the
 * project's counter RNG (the one bp_replay_index and bp_rrt_uniform use); x = left << h | right; repeated while x >= N (cycle walking: the network permutes the
 * 2h-bit domain, so this ends).  -1 for N outside 1 .. 2^31 - 1 or i outside [0, N).
 *
 * Nothing synchronises, nothing is read back; all work is enqueued on `stream`.  BP_EINVAL, before anything is launched: a NULL pointer (boot_ids excepted),
 * row_bytes % 16 != 0, n_steps, num_envs or action_dim < 1, t outside [0, T), K or B < 1, j * B outside [0, N).  (Added within ABI 11: the additions only add.) */
typedef struct bp_rollout_desc {
    int32_t n_steps, num_envs, device, action_dim;
    int64_t row_bytes;
    uint8_t *obs;
    float *action, *reward, *value, *logp, *advantage, *ret;
    uint8_t *episode_start, *last_done;
    int64_t *hdr;
} bp_rollout_desc;
typedef struct bp_rollout_batch {
    float *obs, *action, *value, *logp, *advantage, *ret;
    int32_t *index;
    uint8_t *valid;
} bp_rollout_batch;
int32_t bp_sizeof_rollout_desc(void);
int32_t bp_sizeof_rollout_batch(void);
int64_t bp_rollout_index(uint64_t seed, int64_t epoch, int64_t i, int64_t n);
int bp_rollout_begin(const bp_rollout_desc *d, int32_t t, const uint8_t *obs, const float *action, const float *value, const float *logp, void *stream);
int bp_rollout_pick_rows(const bp_rollout_desc *d, const uint8_t *mask, const uint8_t *src, int32_t K, int32_t *out_ids, float *out_rows, void *stream);
int bp_rollout_end(const bp_rollout_desc *d, int32_t t, const double *reward, const uint8_t *done, const int32_t *boot_ids, const float *boot_values,
                   int32_t K, double gamma, void *stream);
int bp_rollout_finish(const bp_rollout_desc *d, const float *last_values, double gamma, double gl, void *stream);
int bp_rollout_minibatch(const bp_rollout_desc *d, uint64_t seed, int64_t epoch, int32_t j, int32_t B, const bp_rollout_batch *out, void *stream);

/* ---- transition buffer for lock-step envs (DESIGN.md "Transition buffer") ----
 * Handle-free: the caller owns every array (device memory on `device`) and passes them in a bp_transitions_desc.  T = steps, E = num_envs, A = action_dim,
 * R = row_bytes (a multiple of 16; the rows are uint8 and their shape is opaque to the library; every observation array is 16-byte aligned), T * E at most
 * 2^31 - 1.  A ring of T step rows of E envs:
 *   obs, next_obs uint8 [T][E][R]; action float [T][E][A]; reward float [T][E]; done, timeout uint8 [T][E]
 *   hdr int64 [2]: hdr[0] adds ever made, hdr[1] sample draws made
 * All of it starts as zeros.  Transition (s, e), s the number of adds before it, lives in slot (s % T) * E + e.
 *
 * bp_transitions_add writes step row hdr[0] % T (read on the device): obs = obs[e]; next_obs = done[e] ? terminal_obs[e] : next_obs[e] (all uint8
 * [E][R]); action = action (float [E][A]); reward = (float)reward[e] (double [E]); done = done[e] != 0; timeout = done[e] && truncated[e] (uint8 [E]
 * each).  Then hdr[0] grows by one, in a kernel the stream orders after the copies.  The arguments are consumed in stream order: work enqueued on `stream`
 * after the call may rewrite them.
 *
 * bp_transitions_sample draws B transitions with replacement: n = min(hdr[0], T) * E on the device, sample b takes slot bp_replay_index(seed, hdr[1], b, n),
 * then hdr[1] grows by one.  out: obs, next_obs float [B][R] ((float)u8 / 255.0f by IEEE division, 16-byte aligned), action float [B][A], reward float [B],
 * done float [B] = done * (1 - timeout) (a done that the time limit caused does not stop a bootstrap), slot int32 [B], valid uint8 [B] = 1 when n > 0;
 * with n == 0 every output is zero and slot is -1.
 *
 * Nothing synchronises, nothing is read back; all work is enqueued on `stream`.  BP_EINVAL, before anything is launched: a NULL pointer, row_bytes % 16 != 0,
 * steps, num_envs or action_dim < 1, steps * num_envs > 2^31 - 1, B < 1, an observation array that is not 16-byte aligned.  (Added within ABI 11: the
 * additions only add.) */
typedef struct bp_transitions_desc {
    int32_t steps, num_envs, device, action_dim;
    int64_t row_bytes;
    uint8_t *obs, *next_obs;
    float *action, *reward;
    uint8_t *done, *timeout;
    int64_t *hdr;
} bp_transitions_desc;
typedef struct bp_transitions_batch {
    float *obs, *next_obs, *action, *reward, *done;
    int32_t *slot;
    uint8_t *valid;
} bp_transitions_batch;
int32_t bp_sizeof_transitions_desc(void);
int32_t bp_sizeof_transitions_batch(void);
int bp_transitions_add(const bp_transitions_desc *d, const uint8_t *obs, const uint8_t *next_obs, const uint8_t *terminal_obs, const float *action,
                       const double *reward, const uint8_t *done, const uint8_t *truncated, void *stream);
int bp_transitions_sample(const bp_transitions_desc *d, uint64_t seed, int32_t B, const bp_transitions_batch *out, void *stream);

const char *bp_last_error(const bp_handle *h);
int32_t bp_abi_version(void);
int32_t bp_sizeof_config(void);   /* sizeof(bp_config), so a binding can verify its struct layout */

#ifdef __cplusplus
}
#endif
#endif
