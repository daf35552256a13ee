/* drlgx — C ABI of the MI355X-native exploration belief-step / GCN hot path.
 *
 * This is the drop-in boundary: plain C types, opaque handle, int return codes, no
 * torch types.  The reference has no C ABI today — its boundary is two pybind11 modules
 * (`ss2d`: /root/reference/src/SS2D.cpp:18-258, `planner2d`: /root/reference/src/Planner2D.cpp:9-106);
 * each entry point below names the reference interface it replaces.  The Python shims in
 * drl_graph_exploration_amd/ (ss2d.py, planner2d.py, vecenv.py, networks.py) sit on top of it.
 *
 * Conventions
 *  - "dev" pointers are DEVICE (HBM) pointers owned by the caller (e.g. torch tensor data_ptr());
 *    "host" pointers are ordinary host memory.  Every function that takes host pointers says so
 *    in its name (…_host) or parameter comment; those functions synchronise the engine stream.
 *  - All kernels of an engine are enqueued on ONE HIP stream (drlgx_set_stream; default: a private
 *    stream).  Non-_host calls are asynchronous with respect to the host.
 *  - Instance = one belief state.  Instances [0, n_envs) are live environments; the engine owns
 *    additional scratch instances for look-ahead rollouts (one "base" per env + n_rollouts).
 *  - Return value: 0 = OK, <0 = DRLGX_E_* error (see drlgx_strerror).  Nothing aborts.
 *  - There is NO CPU fallback: if no HIP device is present drlgx_create fails with DRLGX_E_NODEVICE.
 */
#ifndef DRLGX_H
#define DRLGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRLGX_OK 0
#define DRLGX_E_INVALID (-1)   /* bad argument */
#define DRLGX_E_NODEVICE (-2)  /* no HIP device / runtime error */
#define DRLGX_E_CAPACITY (-3)  /* an instance overflowed max_poses / max_landmarks / max_factors */
#define DRLGX_E_HIP (-4)       /* HIP runtime error (message in drlgx_last_error) */
#define DRLGX_E_NUMERIC (-5)   /* non-SPD system met by the SLAM solve (gtsam: IndeterminantLinearSystemException) */

#define DRLGX_ALG_EM_AOPT 0 /* Planner2D.h OptimizationAlgorithm::EM_AOPT (trace) */
#define DRLGX_ALG_EM_DOPT 1 /* OptimizationAlgorithm::EM_DOPT (determinant)      */
#define DRLGX_ALG_OG_SHANNON 2      /* OptimizationAlgorithm::OG_SHANNON (map entropy: drlgx_og_cost, drlgx_og_plan) */
#define DRLGX_ALG_SLAM_OG_SHANNON 3 /* OptimizationAlgorithm::SLAM_OG_SHANNON (drlgx_slam_og_cost, drlgx_og_plan)    */

/* Parameters of one engine.  Mirrors the ini sections read by scripts/envs/pyss2d.py:10-55 and
 * scripts/envs/pyplanner2d.py:24-54 (values: scripts/envs/exploration_env.ini). Angles in radians,
 * already wrapped through Rot2(x).theta() as the reference setters do (Simulation2D.h:52-55,152). */
typedef struct drlgx_config {
  /* [Sensor Model]  BearingRangeSensorModel::Parameter (include/em_exploration/Simulation2D.h:47-76) */
  double bearing_noise, range_noise, min_bearing, max_bearing, min_range, max_range;
  /* [Control Model]  SimpleControlModel::Parameter (Simulation2D.h:145-160) */
  double translation_noise, rotation_noise;
  /* [Environment]  unpadded box, Environment::Parameter (Simulation2D.h:243-268) */
  double env_min_x, env_max_x, env_min_y, env_max_y, safe_distance;
  /* map box = environment padded by ext = 20 m (pyss2d.py:48-55) */
  double map_min_x, map_max_x, map_min_y, map_max_y;
  /* [Virtual Map]  VirtualMap::Parameter (include/em_exploration/VirtualMap.h:17-38) */
  double resolution, sigma0; /* resolution >= 1: the reference divides by (int)resolution (VirtualMap.cpp:341) */
  int32_t num_samples; /* only 1 is supported (the shipped value); >1 re-averages identical maps */
  /* [Simulator] */
  double sigma_x0, sigma_y0, sigma_theta0;
  int32_t num_landmarks; /* Simulator.num: ground-truth landmarks sampled per env.  The simulator kernels keep 20 B of LDS per
                          * landmark (24 B in the look-ahead's pre-simulation) beside 5 024 - 7 528 B, within 64 KB:
                          * drlgx_create refuses (DRLGX_E_INVALID) more than 2 900, with n_rollouts > 0 more than 2 521;
                          * drlgx_set_env_obstacles(1) needs 36 B per landmark and refuses more than 1 680 */
  /* [Planner]  EMPlanner2D::Parameter (include/em_exploration/Planner2D.h; src/Planner2D.cpp:26-41) */
  double angle_weight, distance_weight0, distance_weight1, occupancy_threshold, max_edge_length;
  int32_t algorithm; /* DRLGX_ALG_* */
  /* capacities (new: the reference grows std::vectors) */
  int32_t max_poses;     /* P_max per instance (>= 2; any value whose tables fit the 160 KB LDS: drlgx_create checks) */
  int32_t max_landmarks; /* L_max observed landmarks per instance (likewise; no fixed cap) */
  int32_t max_factors;   /* M_max bearing-range factors per instance */
  int32_t max_actions;   /* A_max actions per look-ahead candidate */
  int32_t max_snapshots; /* device-resident snapshot slots of the live environments (0..16) */
} drlgx_config;

typedef struct drlgx_engine drlgx_engine;

/* ---- life cycle ----------------------------------------------------------------------------- */

/* Create an engine with n_envs environments and n_rollouts look-ahead scratch instances on HIP
 * device `device`.  Replaces the constructors ss2d.Simulator2D / SLAM2D / VirtualMap and
 * planner2d.EMPlanner2D (src/SS2D.cpp:173-188,190-211,226-246; src/Planner2D.cpp:75-92). */
int drlgx_create(const drlgx_config *cfg, int n_envs, int n_rollouts, int device, drlgx_engine **out);
int drlgx_destroy(drlgx_engine *e);
/* Use the caller's HIP stream (hipStream_t) for all subsequent work: NULL = HIP's default (null)
 * stream, (void*)-1 = back to the engine's private non-blocking stream (the initial state). */
int drlgx_set_stream(drlgx_engine *e, void *hip_stream);
int drlgx_synchronize(drlgx_engine *e);
const char *drlgx_strerror(int code);
/* Text of the engine's last error; with e = NULL, why this thread's last drlgx_create failed (the engine is gone by then). */
const char *drlgx_last_error(const drlgx_engine *e);
/* Device-side status word of the last kernels: 0 or a DRLGX_E_* code (synchronises). */
int drlgx_status_host(drlgx_engine *e);
/* The same, with `bytes` of device memory copied to the host under the same synchronisation (bytes = 0: drlgx_status_host).  A batched
 * trainer needs a handful of small device results per vector step on the host - counts, offsets, the read-out of the policy
 * (scripts/policy.py:100-127, 392-400 read them one Python attribute at a time); each separate read drains the stream again. */
int drlgx_status_fetch_host(drlgx_engine *e, const void *src_dev, size_t bytes, void *dst_host);

/* ---- SS2D life cycle (scripts/envs/pyss2d.py:58-206) ----------------------------------------- */

/* SS2D.__init__ for `n` environments: seed the three mt19937 streams with seeds[i]
 * (Simulator2D.cpp:436-443), place the vehicle at start_xytheta[i], rejection-sample the landmarks
 * (Simulator2D::addLandmarks, Simulator2D.cpp:445-464), add the prior (SLAM2D::addPrior,
 * SLAM2D.cpp:44-57), first measure + optimize.  env_ids / seeds / start_xytheta are HOST arrays
 * (n, n, n*3).  Resets the virtual map to its untouched state (VirtualMap::initialize). */
int drlgx_reset_host(drlgx_engine *e, int n, const int32_t *env_ids, const uint32_t *seeds,
                     const double *start_xytheta);

/* SS2D.simulate(odom, core=True) for every environment with active[i] != 0 (NULL = all):
 * Simulator2D::move + SLAM2D::addOdometry, two noisy Simulator2D::measure calls (the first only
 * consumes noise: pyss2d.py:182), SLAM2D::addMeasurement, SLAM2D::optimize,
 * VirtualMap::updateProbability + updateInformation.  odom_dev: DEVICE double[n_envs*3]
 * (x, y, theta); active_dev: DEVICE uint8[n_envs] or NULL. */
int drlgx_step(drlgx_engine *e, const double *odom_dev, const uint8_t *active_dev);

/* ExplorationEnv.step (scripts/envs/exploration_env.py:98-105: `for a in actions: self._sim.simulate(a)`) one action
 * index at a time for all envs: env i executes actions[i][action_index] (DEVICE double [n_envs][max_actions][3], the plans
 * drlgx_line_plan emits) while action_index < n_actions[i].  map_last_only != 0: the virtual map - a pure function of the
 * SLAM state - is rebuilt at each env's last action only (and the marginal covariances only where the map needs them);
 * the state after the plan is the same, intermediate getters of the map see the previous rebuild. */
int drlgx_step_plan(drlgx_engine *e, const double *actions_dev, const int32_t *n_actions_dev, int action_index,
                    int map_last_only);
/* The same loop for ALL action indices in one call: env i executes actions[i][0 .. n_actions[i]); max_n_actions: a host-side
 * bound of the plan lengths (<= max_actions).  A workgroup runs its env's whole plan inside one launch wherever a fused step
 * kernel serves the pose counts the plans reach (one launch for the actions the dense-solver step serves, one for the rest
 * around the pose-chain solver: the same per-action choice as drlgx_step_plan makes), else one drlgx_step_plan per action
 * index; bit-equal either way. */
int drlgx_step_plans(drlgx_engine *e, const double *actions_dev, const int32_t *n_actions_dev, int max_n_actions,
                     int map_last_only);
/* The same loop as the reference's evaluation script runs it (scripts/test.py:128-152): per executed action a record of the
 * metrics, and the episode ends in the MIDDLE of a plan when ExplorationEnv.step reports done.  For every action index a in
 * [0, max_n_actions): what drlgx_step_plan(e, actions, n_actions, a, 0) launches (the map is rebuilt at every action), then one
 * record launch: for every env with a < n_actions[e], trace_dev[e][a] = (landmark error, map entropy, max localisation
 * uncertainty - the bits of drlgx_metrics with this sigma0 -, explored - the bits of drlgx_explored), and when
 * explored > done_explored || step > max_steps (exploration_env.py:107-110) done_dev[e] = 1 and n_actions_dev[e] = a + 1, so
 * that the later action indices skip the env without a host round trip.  After the call n_actions_dev (IN and OUT) holds the
 * number of actions each env executed; rows of trace_dev beyond it are not written.  done_dev is only ever set: the caller
 * zeroes it.  trace_dev double [n_envs][max_actions][4], done_dev int32 [n_envs]. */
int drlgx_step_plans_traced(drlgx_engine *e, const double *actions_dev, int32_t *n_actions_dev, int max_n_actions, double sigma0,
                            double done_explored, int max_steps, double *trace_dev, int32_t *done_dev);

/* SS2D.simulate's obstacle flag (scripts/envs/pyss2d.py:132,180-197,206), an OPT-IN (default 0): existing callers pass the ini
 * files' non-zero [Environment] safe_distance and rely on it being inert.  With enabled != 0 and cfg.safe_distance > 0 every belief
 * step of the live envs (drlgx_step, drlgx_step_plan, drlgx_step_plans, drlgx_step_plans_traced, drlgx_follow_plans) also decides,
 * for a step that moves, over the measurements of the step's FIRST measure() call that pass the sensor gates (noisy values):
 *   obstacle = any(range < cfg.safe_distance && (cleared || the key has no landmark slot before this step's appends)),
 *   cleared  = !obstacle
 * (the reference stops at the first hit; no branch of its scan does anything else, so the rule does not depend on the order).  A
 * rejected odometry draws nothing, reports obstacle = 0 and leaves cleared alone; an env switched off keeps both.  After a reset:
 * obstacle 0, cleared 1.  Both are instance state: snapshots, restores (lazy or not) and instance copies carry them.  The draws,
 * their order and everything the step appends are unchanged: beliefs, maps and random streams are bit-equal to the same steps
 * without the opt-in.  Under the opt-in the step runs as the three stage kernels (timers 0-2, not 5), drlgx_step_plans as one
 * drlgx_step_plan per action index.  Look-ahead rollouts (drlgx_lookahead, drlgx_em_cost ...) have no obstacle logic
 * (Planner2D.cpp:1432-1460) and neither read nor write the flags.  Off, or with cfg.safe_distance <= 0: nothing changes, the flags
 * keep their last values.  DRLGX_E_CAPACITY (the opt-in stays off, plain steps go on as before): enabled != 0 on an engine with more
 * than 1 680 listed landmarks - the flag's simulator stage keeps both measure() calls' variates in LDS, 36 num_landmarks + 5 024 B,
 * and its launch stays within 64 KB. */
int drlgx_set_env_obstacles(drlgx_engine *e, int enabled);
/* out_dev: DEVICE uint8 [2][n_envs] - plane 0 the last step's obstacle flag, plane 1 cleared. */
int drlgx_obstacle_flags(drlgx_engine *e, uint8_t *out_dev);

/* Follow a plan (EMExplorer.follow_path and the switch on the planner's result in explore(), scripts/envs/pyplanner2d.py:100-109,
 * 170-187), all envs, no host round trip.  One selection launch decides what env i executes from result_dev[i]
 * (EMPlanner2D::OptimizationResult as drlgx_em_plan reports it):
 *   3 SUCCESS            the first min(steps, n_actions_dev[i]) rows of plan_dev[i];
 *   0 SAMPLING_FAILURE   one action, fallback_xytheta (HOST double[3]; the reference's (0, 0, pi/4)), whatever `steps` is;
 *   1 NO_SOLUTION / 2 TERMINATION, or active_dev[i] == 0 (NULL: all active): nothing.
 * Execution is drlgx_step_plans_traced's: per action index one belief step (the map rebuilt every time) and one record launch that
 * writes trace_dev[i][a] (same four columns, same bits) and cuts env i behind action a when
 *   explored > done_explored || step > max_steps  (done_dev[i] = 1),            stop 1
 *   else the step raised the obstacle flag (drlgx_set_env_obstacles),           stop 2 - the step stays executed and recorded
 *   else env i's next action is a rejected odometry (outside the map box),      stop 3 - it is not executed and writes no row;
 * a rejected FIRST action is cut by the selection launch.  stop_dev[i]: 0 ran its actions (none, for an inactive env), 1 done,
 * 2 obstacle, 3 rejected odometry, 4 no solution, 5 termination.  n_exec_dev[i] (OUT): the actions executed = rows written.
 * Without the obstacle opt-in the call never stops for an obstacle.  plan_dev double [n_envs][max_actions][3] and n_actions_dev
 * int32 [n_envs] are only read; trace_dev double [n_envs][max_actions][4]; n_exec_dev, done_dev (only ever set: the caller zeroes
 * it), stop_dev int32 [n_envs].  All DEVICE but the fallback. */
int drlgx_follow_plans(drlgx_engine *e, const double *plan_dev, const int32_t *n_actions_dev, const int32_t *result_dev,
                       const uint8_t *active_dev, int steps, const double *fallback_xytheta, double sigma0, double done_explored,
                       int max_steps, double *trace_dev, int32_t *n_exec_dev, int32_t *done_dev, int32_t *stop_dev);

/* ---- staged form of the belief step -----------------------------------------------------------
 * The reference's pybind classes are driven call by call (scripts/envs/pyss2d.py:102-138 SS2D.__init__, :171-206
 * SS2D.simulate); the object-level shims (drl_graph_exploration_amd/ss2d.py) map every such call onto one of these.
 * drlgx_step == stage_move; stage_measure (discarded); stage_measure + stage_add_measurements; stage_optimize;
 * stage_update_map, fused.  All buffers are DEVICE memory; active_dev: uint8[n_envs] or NULL (= all). */
/* SS2D.__init__ up to SLAM2D::addPrior (src/SS2D.cpp:173-176 Simulator2D(...), initialize_vehicle, random_landmarks;
 * :191 SLAM2D::add_prior): like drlgx_reset_host but WITHOUT the first measure / optimise / map reductions. */
int drlgx_stage_reset_host(drlgx_engine *e, int n, const int32_t *env_ids, const uint32_t *seeds, const double *start_xytheta);
/* SLAM2D::add_prior(VehicleBeliefState(pose, information)) with a FULL information matrix (src/SS2D.cpp:191,
 * SLAM2D.cpp:44-57: noiseModel::Gaussian::Information): replaces the prior information of one env - the diagonal of the
 * ini file's sigma_x0 / sigma_y0 / sigma_theta0 that the resets install - after drlgx_stage_reset_host and before the first
 * optimise.  HOST, row major 3 x 3, symmetric (DRLGX_E_INVALID otherwise). */
int drlgx_stage_set_prior_information_host(drlgx_engine *e, int env, const double *information9);
/* SLAM2D::add_prior(VehicleBeliefState(pose, information)) with a POSE that is not the simulator's initial vehicle pose
 * (src/SS2D.cpp:193, SLAM2D.cpp:44-57: the pose of the prior factor AND the initial estimate of x0; the reference's own caller,
 * pyss2d.py:124-135, passes the vehicle's pose - what the resets install): replaces it for one env, between
 * drlgx_stage_reset_host and the first measurement (one pose, no factor: DRLGX_E_INVALID otherwise).  HOST, (x, y, theta). */
int drlgx_stage_set_prior_pose_host(drlgx_engine *e, int env, const double *xytheta);
/* Simulator2D::move(odom, true) (src/SS2D.cpp:181) + SLAM2D::add_odometry (:193). odom_dev: double[n_envs*3]. */
int drlgx_stage_move(drlgx_engine *e, const double *odom_dev, const uint8_t *active_dev);
/* Simulator2D::measure() (src/SS2D.cpp:182): the noisy (bearing, range) of every ground-truth landmark that passes the
 * sensor gates, in the reference's iteration order; advances the sensor RNG; adds nothing to the graph.
 * keys_dev: int32[n_envs*num_landmarks], bearing_range_dev: double[n_envs*num_landmarks*2], count_dev: int32[n_envs]. */
int drlgx_stage_measure(drlgx_engine *e, const uint8_t *active_dev, int32_t *keys_dev, double *bearing_range_dev, int32_t *count_dev);
/* SLAM2D::add_measurement(key, m) (src/SS2D.cpp:194) for count[i] listed measurements of env i at its newest pose. */
int drlgx_stage_add_measurements(drlgx_engine *e, const uint8_t *active_dev, const int32_t *keys_dev, const double *bearing_range_dev,
                                 const int32_t *count_dev);
/* SLAM2D::optimize(update_covariance = true) (src/SS2D.cpp:198). */
int drlgx_stage_optimize(drlgx_engine *e, const uint8_t *active_dev);
/* rebuild != 0: VirtualMap::update_probability(slam, sensor) + update_information(map, sensor) (src/SS2D.cpp:228-235);
 * rebuild == 0: only the utility / explored sums of the stored planes (the state a freshly constructed VirtualMap is in). */
int drlgx_stage_update_map(drlgx_engine *e, const uint8_t *active_dev, int rebuild);

/* FastMarginals2::update / propagate (src/em_exploration/FastMarginals.cpp:188-321) fed as the EM planner feeds it
 * (src/em_exploration/Planner2D.cpp:652-737 updateNodeInformation_EM, :472-551 updateTrajectory_EM): for n_cand
 * candidates (environment, action list) the 3x3 marginal covariance of EVERY pose after appending one predicted
 * (noise-free) pose per action and the noise-free bearing-range factors from the new poses to the landmarks of the
 * estimated map that pass the sensor gates - an EKF-style propagate / update, Sigma' = Sigma - Sigma A^T (I + A Sigma
 * A^T)^-1 A Sigma, without re-solving and without touching the environments' state.
 * cand_env_dev int32[n_cand]; actions_dev double[n_cand*max_actions*3]; n_actions_dev int32[n_cand];
 * cov_out_dev double[n_cand*out_stride_poses*9] (row-major 3x3 per pose: the P old poses, then one per action),
 * out_stride_poses >= max_poses + max_actions; n_out_dev int32[n_cand] = P + n_actions.  At most 256 predicted
 * measurements per candidate (DRLGX_E_CAPACITY beyond). */
int drlgx_fm2_update(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                     double *cov_out_dev, int out_stride_poses, int32_t *n_out_dev);
/* drlgx_fm2_update for action lists with NON-CORE steps, as the edges of the Dubins control model have them (Planner2D.cpp:659-682,
 * :714-731): core_dev uint8[n_cand*max_actions] marks the actions that are core poses; NULL = every action, and the call is then
 * drlgx_fm2_update (the same kernel, the same bits).  Every action still appends its predicted pose and its odometry factor - the
 * chain of covariances runs through every step -, but only a core pose predicts measurements, so the 256-measurement capacity
 * applies to the masked count.  cov_out_dev holds one 3x3 block per pose as before, the P old poses and EVERY step, each with the
 * full update Sigma' applied (the reference's FastMarginals2::update corrects the blocks of `updated_keys` only - the old poses and
 * each edge's last pose - and leaves the intermediate steps at their propagated covariance, which nothing reads; for those steps
 * this entry returns the posterior marginal instead).  Any mask is legal, trailing non-core steps included. */
int drlgx_fm2_update_steps(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                           const uint8_t *core_dev, double *cov_out_dev, int out_stride_poses, int32_t *n_out_dev);
/* The leaf evaluation of EMPlanner2D::optimize2 (src/em_exploration/Planner2D.cpp:1095-1104) for n_cand candidates (environment,
 * action list) the caller supplies (drlgx_em_plan below grows optimize2's tree and feeds its leaves to this entry's body):
 *   updateTrajectory_EM (:472-551): the covariances of drlgx_fm2_update; every pose becomes a core pose of the leaf's map with
 *     information = cov^-1 (:521-523), the old ones at the current estimate (:1288), one per action at the noise-free predicted pose;
 *   VirtualMap::updateInformation on a copy of the root's virtual map (:1100-1101; VirtualMap.cpp:256-316, :213-229, :364-378):
 *     every cell back to I / sigma0^2, the poses in trajectory order, first hit replaces, later hits are fused by covariance
 *     intersection; the cells' probabilities stay the live environment's;
 *   calculateUncertainty_EM (:321-341): sum_v 1[p_v > 0.49] tr(info_v^-1) (DRLGX_ALG_EM_AOPT) or sum_v 1[p_v > 0.49] / det(info_v)
 *     (DRLGX_ALG_EM_DOPT);
 *   costFunction (:418-420) = uncertainty + distance * distance_weight, distance_weight = w0 - (w0 - w1) #{p_v <
 *     occupancy_threshold} / V (:1322-1332), distance = sum_k sqrt(x_k^2 + y_k^2 + angle_weight theta_k^2) as drlgx_lookahead
 *     accumulates it (:1440).
 * A plan is ranked by that scalar without simulating it, without noise and without re-solving; live environments are not modified.
 * cand_env_dev int32[n_cand] (several candidates may name one environment); actions_dev double[n_cand*max_actions*3];
 * n_actions_dev int32[n_cand], 0 <= n <= max_actions; uncertainty_out_dev / cost_out_dev: DEVICE double[n_cand], either may be NULL
 * but not both; info_out_dev: DEVICE double[n_cand*V*3] (xx, xy, yy per cell, row-major grid: the leaf virtual map's information) or
 * NULL.  Any n_cand >= 0.  DRLGX_E_INVALID: a bad algorithm, both outputs NULL, a candidate that names no environment or has more
 * than max_actions actions; DRLGX_E_CAPACITY: more than 256 predicted measurements in one candidate.  The candidates are checked
 * before anything else is launched (one read of a device flag: this call synchronises once); a refused call leaves the status word
 * alone. */
int drlgx_em_cost(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                  int algorithm, double *uncertainty_out_dev, double *cost_out_dev, double *info_out_dev);
/* drlgx_em_cost for the leaves of a tree whose edges have NON-CORE steps (the Dubins control model: updateNodeInformation_EM,
 * Planner2D.cpp:659-682, adds one odometry factor and one pose per step, predicts measurements at the edge's last pose only, :714-731,
 * and updateTrajectory_EM puts only that last pose into the leaf's map, :498, :514-524):
 *   core_dev uint8[n_cand*max_actions] or NULL (= every action is a core pose): the covariances are those of
 *     drlgx_fm2_update_steps; the leaf's map holds the P old poses and the CORE new poses only - a non-core step is marked skipped
 *     before its information is factored, so it can never raise DRLGX_E_NUMERIC -, while the pose chain still composes every row;
 *   distance_dev double[n_cand] or NULL: the leaf's distance as the tree accumulated it (v dt n + |w dt n| angle_weight per edge,
 *     :293-303), used in the cost instead of sum_k sqrt(x_k^2 + y_k^2 + angle_weight theta_k^2).
 * With both NULL the call is drlgx_em_cost: the same kernels, the same bits.  Everything else - the other arguments, the checks
 * before anything is launched (the 256-measurement capacity counts the predicted measurements of core poses only), the single
 * synchronisation, a refused call leaving live state and the status word alone - is drlgx_em_cost's.  Any mask is legal, trailing
 * non-core steps included. */
int drlgx_em_cost_steps(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                        const uint8_t *core_dev, const double *distance_dev, int algorithm, double *uncertainty_out_dev,
                        double *cost_out_dev, double *info_out_dev);

/* calculateUncertainty_OG_SHANNON (src/em_exploration/Planner2D.cpp:368-392) and costFunction (:418-420) for n_cand candidates
 * (environment, action list) the caller supplies - the Shannon entropy of the occupancy map after the plan's poses have swept it:
 *   OccupancyMap::update(map) (OccupancyMap.cpp:122-138): every cell at LOGODDS_UNKNOWN; one occupied update of its cell per estimated
 *     landmark inside the grid; then every pose in trajectory order - the P old poses at the current estimate, one per action at the
 *     noise-free predicted pose chained from the last estimate (as drlgx_em_cost chains them) - updates the cells of its sector-sweep
 *     bounding box that pass checkWithoutMinRange and are not at MIN_LOGODDS: occupied above OCCUPIED_THRESH + 1e-8, else free;
 *   p_v = the cell's probability (VirtualMap::updateProbability, VirtualMap.cpp:61-84); entropy = sum_v -p_v ln p_v - (1 - p_v) ln(1 - p_v);
 *   cost = entropy + distance * distance_weight, both exactly drlgx_em_cost's (the distance weight from the LIVE map's probabilities).
 * No covariance is needed, nothing is simulated or re-solved, live environments are not modified.  (The reference's tree planners
 * cannot run under OG_SHANNON as shipped - Node::map stays a null pointer, Planner2D.h:92, Planner2D.cpp:256, :785 - so this is the
 * cost's arithmetic for caller-supplied plans, which drlgx_og_plan applies to the leaves of optimize2's tree; drlgx_em_plan and
 * drlgx_em_cost's algorithms are unchanged, SLAM_OG_SHANNON is drlgx_slam_og_cost.)
 * Candidate layout as drlgx_em_cost: cand_env_dev int32[n_cand] (several candidates may name one environment); actions_dev
 * double[n_cand*max_actions*3]; n_actions_dev int32[n_cand], 0 <= n <= max_actions.  entropy_out_dev / cost_out_dev: DEVICE
 * double[n_cand], either may be NULL but not both; prob_out_dev: DEVICE double[n_cand*V] (row-major grid: the leaf map's
 * probabilities) or NULL.  Any n_cand >= 0 (0 returns at once and reads no array), all candidates in one launch.  DRLGX_E_INVALID: both scalar outputs NULL, a candidate
 * that names no environment or has more than max_actions actions.  The candidates are checked before anything else is launched (one
 * read of a device flag: this call synchronises once); a refused call leaves the status word and the live state alone. */
int drlgx_og_cost(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                  double *entropy_out_dev, double *cost_out_dev, double *prob_out_dev);

/* calculateUncertainty_SLAM_OG_SHANNON (src/em_exploration/Planner2D.cpp:394-416) and costFunction (:418-420) for n_cand candidates
 * (environment, action list) the caller supplies - the fourth OptimizationAlgorithm (include/em_exploration/Planner2D.h:32-37), the
 * one that weighs map entropy against landmark uncertainty:
 *   updateTrajectory_SLAM_OG_SHANNON (:584-618) adds the plan's noise-free odometry and predicted bearing-range factors to a copy of
 *     the root's iSAM2 and reads every landmark's marginal covariance (:608-611).  With zero residuals and no relinearisation that is
 *     the linear update of drlgx_fm2_update, Sigma' = Sigma - Sigma A^T (I + A Sigma A^T)^-1 A Sigma, read on the LANDMARK diagonal
 *     blocks (the one deviation: iSAM2's update may relinearise variables past its threshold, the linear update does not);
 *   slam_uncertainty = sum_l sqrt(det Sigma'(l, l)) over the environment's landmarks in slot order (:409-413);
 *   H_leaf = drlgx_og_cost's entropy of the same candidate (:397-407; the same kernel, the same bits);
 *   the root's weights, once per call and environment from the LIVE belief (EMPlanner2D::initialize, :1341-1354):
 *     w2 = (1 - alpha) / H_root, H_root the Shannon entropy of the live virtual map's probabilities;
 *     w1 = alpha / sum_l sqrt(det(inverse(information_l))) over the live landmark marginals (what drlgx_get_landmarks_host returns);
 *     both divisions are plain IEEE as in the reference: an environment without a landmark has w1 = inf (alpha > 0) or NaN
 *     (alpha = 0), and its candidates' uncertainty is inf * 0 = NaN - nothing is special-cased;
 *   uncertainty = w2 H_leaf + w1 slam_uncertainty (:407, :413); cost = uncertainty + distance * distance_weight, distance and
 *     distance_weight exactly drlgx_og_cost's.
 * Candidates as drlgx_em_cost_steps: cand_env_dev int32[n_cand], actions_dev double[n_cand*max_actions*3], n_actions_dev
 * int32[n_cand]; core_dev uint8[n_cand*max_actions] or NULL (= every action is a core pose): only core poses predict measurements
 * (the entropy sweep still takes every pose, as drlgx_og_cost does); distance_dev double[n_cand] or NULL (= the plan's own distance,
 * as drlgx_og_cost computes it).  alpha in [0, 1] (EMPlanner2D::Parameter::alpha, Planner2D.h:75).
 * uncertainty_out_dev / cost_out_dev: DEVICE double[n_cand], both required.  Optional (NULL = not wanted): terms_out_dev
 * double[n_cand*2] (H_leaf, slam_uncertainty); weights_out_dev double[n_envs*2] (w1, w2); lm_cov_out_dev
 * double[n_cand*max_landmarks*3] (xx, xy, yy of Sigma'(l, l) per slot; slots beyond the environment's landmark count are not written).
 * A candidate that predicts no measurement gets the prior blocks unchanged.  The same call on the same belief returns the same bits
 * (the prior covariance is summed in a fixed order here, unlike drlgx_fm2_update's).
 * DRLGX_E_INVALID: a NULL required pointer, n_cand <= 0, alpha outside [0, 1], a candidate that names no environment or has more than
 * max_actions actions; DRLGX_E_CAPACITY: more than 256 predicted measurements in one candidate (of core poses, with a mask).  The
 * candidates are checked before anything else is launched, as drlgx_em_cost checks them (this call synchronises once); a refused call
 * leaves the outputs, the status word and the live state alone.  Candidates go through the update in chunks of 128. */
int drlgx_slam_og_cost(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                       const uint8_t *core_dev, const double *distance_dev, double alpha, double *uncertainty_out_dev,
                       double *cost_out_dev, double *terms_out_dev, double *weights_out_dev, double *lm_cov_out_dev);

/* The planner parameters only the tree sampler reads (EMPlanner2D::Parameter, scripts/envs/pyplanner2d.py:29, :35, :50): max_nodes
 * (the fraction of the known cells that optimize2's tree may hold; >= 0), safe_distance and dubins_control_model_enabled.  The
 * sampler serves safe_distance = 0 and the non-Dubins control model only: other values are stored here and refused by
 * drlgx_em_plan / drlgx_rrt_plan (a safe_distance > 0 is served once drlgx_set_sampler_obstacles, below, has opted in; the Dubins
 * control model is served by drlgx_rrt_plan once drlgx_set_dubins_library_host, below, has loaded a library, and by drlgx_em_plan
 * once drlgx_set_dubins_leaf_scoring has opted in as well).  After
 * drlgx_create: max_nodes 0.5, safe_distance 0, Dubins off. */
int drlgx_set_sampler_parameter(drlgx_engine *e, double max_nodes, double safe_distance, int dubins_control_model_enabled);
/* The sampler's obstacle logic, an OPT-IN (default 0: every call behaves as described above and below, a non-zero safe_distance is
 * refused).  With enabled != 0, drlgx_em_plan / drlgx_rrt_plan accept safe_distance >= 0 (a negative value and the Dubins control
 * model are still refused with DRLGX_E_INVALID before anything is touched; at exactly 0 the plain growth loop runs) and the tree
 * kernel adds, for the non-Dubins control model (src/em_exploration/Planner2D.cpp):
 *   isSafe(node) (:48-56; Distance.cpp:78-97): a point is unsafe iff an estimated landmark of the environment lies strictly nearer
 *     than safe_distance; a negative radius finds nothing;
 *   sampleNode (:101-125): Halton points are drawn until one is safe, every drawn point advances the index; more than 1000 unsafe
 *     points in one sampleNode end the tree with SAMPLING_FAILURE;
 *   isSafe(node, parent) in connectNode, on the scaled child (:58-86, :243-248): safe if |safe_distance| < 1e-3; else with
 *     d = range(child, parent) and unit = the child's position in the parent's frame / d, the points child.transform_from(l unit)
 *     for l = sd/2; l < d; l += sd/2 must all be safe.  As the reference writes it these points lie BEYOND the child along the
 *     child's heading, not between parent and child; reproduced as written;
 *   the connect counter (:1070-1079, :890-899): a refused connect adds no node; more than 1000 in a row end the tree with
 *     SAMPLING_FAILURE;
 *   the shrink at the start of a call (:1046-1054, :841-849): if the current pose estimate is nearer than safe_distance to its
 *     nearest estimated landmark, the call runs with distance - 0.1 (drlgx_em_plan: max(0, .); drlgx_rrt_plan: unclamped) - but, as
 *     in the reference, only if that landmark's KEY is smaller than the NUMBER of landmarks (searchLandmarkNearest returns the key,
 *     Simulator2D.cpp:394-403, nearest in key order with strict <; the planner compares it with getLandmarkSize()).  The stored
 *     parameter is not changed;
 *   rrt_planner's goal edge (:910-922): a goal whose edge is unsafe is not in the tree - result SUCCESS, n_actions 0, the goal not
 *     counted in n_nodes.
 * One deviation: in rrt_planner a shrunk safe_distance below -1e-3 makes the reference's waypoint loop run for ever; the engine ends
 * that tree at once with SAMPLING_FAILURE, an empty plan and its Halton index unchanged.
 * A tree that ends with SAMPLING_FAILURE reports result 0, n_actions 0, no leaves, the nodes accepted so far in n_nodes / nodes_out,
 * and in halton_next the index after the last drawn point; the other trees of the call are not concerned, it offers no candidate to
 * the scoring, and the status word is untouched: a sampling failure is a result, not an error.  optimize (RRT*)
 * stays out of scope; drlgx_og_plan (optimize2 under OG_SHANNON / SLAM_OG_SHANNON) serves the same obstacle logic.  Dubins paths are served for drlgx_rrt_plan, and for drlgx_em_plan behind
 * drlgx_set_dubins_leaf_scoring (below) - not for drlgx_og_plan. */
int drlgx_set_sampler_obstacles(drlgx_engine *e, int enabled);
/* The Dubins control model's path library (EMPlanner2D::initializeDubinsPathLibrary, Planner2D.cpp:1359-1414), and with it the
 * OPT-IN of that control model: with no library loaded the Dubins flag of drlgx_set_sampler_parameter is refused as before.
 * params: HOST double[9] = max_w, dw, min_v, max_v, dv, dt, min_duration, max_duration, tolerance_radius (the [Dubins] section of the
 * planner's ini file, EMPlanner2D::DubinsParameter); NULL clears the library.  The engine builds the library in doubles with the
 * reference's loops, in the reference's order - v from max_v while v > min_v - 1e-10 by v -= dv; w from 0 while w < max_w + 1e-10
 * by w += dw; sign -1 then +1 (w = 0 is listed twice, as -0 and +0); from Pose2(0, 0, 0) and t = 0, while t < max_duration:
 * num_steps++, x += v dt cos(theta), y += v dt sin(theta), theta = atan2(sin, cos) + sign w dt (the angle goes through (cos, sin)
 * at every step, as Pose2(x, y, theta) takes it), t += dt, and an entry {v, sign w, num_steps, end = the pose} whenever
 * t > min_duration (strict).  The counts come from that repeated addition, not from a division.
 * DRLGX_E_INVALID: a non-positive or non-finite max_w, dw, dv, dt or tolerance_radius, max_v < min_v, or parameters that give no
 * entry.  DRLGX_E_CAPACITY: more than 131 072 entries (the shipped [Dubins] section gives 78 030), a path of more than 4 096
 * steps, or more than 2^20 (v, w) pairs; the library loaded before is then kept.
 * With a library loaded and the Dubins flag set, drlgx_rrt_plan is served at safe_distance = 0, or >= 0 under
 * drlgx_set_sampler_obstacles; drlgx_em_plan still returns DRLGX_E_INVALID unless drlgx_set_dubins_leaf_scoring, below, has opted
 * in (the reference's Dubins edges have non-core steps, which only drlgx_em_cost_steps scores).  What changes in the tree
 * (Planner2D.cpp):
 *   sampleNode (:41-45, :110-115): the same x, y (Halton bases 2 and 3); the sample's theta is 0 and is not read;
 *   connectNodeDubinsPath (:157-176): local = the sample in the parent's frame; the FIRST entry in library order with
 *     |local - end_i| < tolerance_radius (strict) wins; the node's poses are num_steps Euler steps of that (v, w) from the parent's
 *     pose, the node is the last of them; no entry: the connect is refused;
 *   connectNode (:179-265): no scaling to max_edge_length, no bearing test; isSafe(node, parent) (:59-70): safe at once if
 *     |safe_distance| < 1e-3, else poses 1 .. num_steps - 2 must each pass isSafe(point) - the first and the last are not tested;
 *     distance = parent.distance + v dt n + |w dt n| angle_weight (:295-300); key = parent.key + n: a node's depth counts steps;
 *   a refused connect counts towards the 1001 in a row that end the tree with SAMPLING_FAILURE, at safe_distance = 0 too;
 *   the goal edge (:915): the goal joins the tree only if a library path from the node that reached it ends within
 *     tolerance_radius of the goal and is safe - the goal node is then that path's last pose; otherwise the result is SUCCESS with
 *     n_actions 0, as for a refused goal edge;
 *   the shrink of drlgx_rrt_plan is unclamped as before; there is no waypoint loop, so a negative shrunk safe_distance is served
 *     (a negative radius finds no landmark).
 * The plan (Edge::getOdoms, Planner2D.h:143-151) has one row per STEP, root -> goal: between(previous pose, this pose); n_actions
 * is the total number of steps, and a path of more steps than max_actions refuses the call with DRLGX_E_CAPACITY (live state and
 * the status word untouched).  nodes_out keeps 8 columns: x, y, theta, parent, distance as before, columns 5-7 are (library index,
 * num_steps, 0) instead of an edge odometry. */
int drlgx_set_dubins_library_host(drlgx_engine *e, const double *params);
/* The library as loaded: *n_out = its size (0: none); up to `capacity` entries of end_xytheta [.][3], v, w, num_steps (HOST arrays,
 * each may be NULL). */
int drlgx_dubins_library(drlgx_engine *e, int capacity, int32_t *n_out, double *end_xytheta, double *v, double *w, int32_t *num_steps);
/* The library scan's exact pre-filter (default on): a sample whose position in the parent's frame lies farther from the origin than
 * (the largest |end_i| + tolerance_radius)(1 + 2^-30) cannot match any entry (triangle inequality), so the scan is skipped.
 * enabled = 0 scans every time; the results are identical (tests compare them). */
int drlgx_set_dubins_prefilter(drlgx_engine *e, int enabled);
/* drlgx_em_plan under the Dubins control model, an OPT-IN (default 0: drlgx_em_plan with the Dubins flag set returns
 * DRLGX_E_INVALID as before).  With enabled != 0, a library loaded and the Dubins flag set, drlgx_em_plan is served at
 * safe_distance = 0, or >= 0 under drlgx_set_sampler_obstacles; with enabled != 0 and NO library it returns DRLGX_E_INVALID and
 * touches nothing.  The tree is the Dubins tree described at drlgx_set_dubins_library_host with optimize2's stop rule (max_nodes_
 * accepted nodes; the connect counter of 1000 runs at safe_distance = 0 too, so a tree can end with SAMPLING_FAILURE) and
 * optimize2's shrink (max(0, distance - 0.1), Planner2D.cpp:1046-1054).  Every leaf, in node order, becomes a candidate of
 * drlgx_em_cost_steps: one row per STEP root -> leaf (between(previous pose, this pose)), the core mask 1 at each edge's last step,
 * and the leaf's tree distance; the pick is drlgx_em_plan's.  plan_out_dev / n_actions_out_dev then hold the best leaf's per-step
 * rows; nodes_out columns 5-7 are (library index, num_steps, 0).  A leaf of more steps than max_actions refuses the whole call
 * with DRLGX_E_CAPACITY before anything is written.  Executing non-core steps (simulate(core = false)) and optimize (RRT*) stay
 * out of scope. */
int drlgx_set_dubins_leaf_scoring(drlgx_engine *e, int enabled);
/* The leaves the last served drlgx_em_plan or drlgx_og_plan handed to its scoring, in candidate order (tree by tree, each tree's leaves in node
 * order): *n_out_host = their number, *has_steps_out_host (may be NULL) = 1 if that call ran the Dubins control model - whatever the
 * sampler's flag says now -, else 0; up to `capacity` of them are copied on the engine's stream into the DEVICE arrays (each may
 * be NULL) cand_env int32[.], actions double[.*max_actions*3], n_actions int32[.], core uint8[.*max_actions] (all ones without the
 * Dubins control model), distance double[.] (only after a call with steps: otherwise DRLGX_E_INVALID before anything is written -
 * the cost then took the plan's own distance), cost double[.].  Part of the facade path: under the Dubins control model the plan's
 * rows are per-step odometries, not node columns, and EMPlanner2D / EMExplorer find the picked leaf's node for iter_solution() by
 * comparing the plan with these rows; feeding the leaves to drlgx_em_cost_steps reproduces the costs bit for bit (the tests do).
 * After drlgx_og_plan: no steps, core all ones, no distance, and cost is the cost that call computed - feeding the leaves to
 * drlgx_og_cost (algorithm 2) or to drlgx_slam_og_cost with the same alpha (algorithm 3) reproduces it bit for bit. */
int drlgx_em_plan_leaves(drlgx_engine *e, int capacity, int32_t *n_out_host, int32_t *has_steps_out_host, int32_t *cand_env_out_dev,
                         double *actions_out_dev, int32_t *n_actions_out_dev, uint8_t *core_out_dev, double *distance_out_dev,
                         double *cost_out_dev);
/* EMPlanner2D::optimize2 (src/em_exploration/Planner2D.cpp:1043-1128) for the n_sel environments env_sel_dev names: per environment
 * one tree grown on the device from its live belief (k_em_tree.hip) -
 *   initialize (:1281-1357): root = the current pose estimate; max_nodes_ = floor(#{p_v < occupancy_threshold} * max_nodes);
 *   sampleNode (:101-125): Halton point number count++ (radical inverse in bases 2, 3, 5), x and y over the map box
 *     (map_min_x .. map_max_x, map_min_y .. map_max_y), count starting at halton_start[i];
 *   nearestNode (:267-276; Distance.cpp:5-9, :24-35): arg-min of range^2 + (angle_weight * bearing)^2 from the tree node's frame,
 *     strict <: the lowest node index wins a tie;
 *   connectNode, non-Dubins (:188-216, :250-258): angle = the sample's relative bearing in the parent's frame, len = min(d,
 *     max_edge_length), child = parent * Pose2(angle, (len cos angle, len sin angle)), edge odometry (len cos angle, len sin angle,
 *     angle), distance = parent.distance + sqrt(sqDistanceBetweenPoses(child, parent, angle_weight));
 *   until max_nodes_ nodes are accepted (:1058-1092) -
 * then every leaf (a node without children, in node order; the root itself when max_nodes_ = 0) is scored by the body of
 * drlgx_em_cost with `algorithm`, and the first leaf with the strictly smallest cost is the plan (:1095-1111; the first leaf is
 * always taken, a NaN cost never replaces a held one).  Live environments are only read.
 * Every array is DEVICE memory: env_sel_dev int32[n_sel]; halton_start_dev int32[n_sel] (>= 0); plan_out_dev
 * double[n_sel*max_actions*3] (the best leaf's edge odometry root -> leaf, zero behind the plan); n_actions_out_dev int32[n_sel];
 * cost_out_dev double[n_sel] or NULL; result_out_dev int32[n_sel] or NULL (EMPlanner2D::OptimizationResult: 0 SAMPLING_FAILURE,
 * 1 NO_SOLUTION, 2 TERMINATION, 3 SUCCESS - optimize2 at safe_distance 0 always succeeds); n_leaves_out_dev int32[n_sel] or NULL;
 * halton_next_out_dev int32[n_sel] or NULL: the Halton index after the call (the reference's sequence keeps counting from call to
 * call); nodes_out_dev double[n_sel*max_tree_nodes*8] or NULL: per node x, y, theta, parent index (-1: the root), distance, and the
 * edge odometry from the parent (x, y, theta; zero for the root) - a leaf's plan is its ancestors' edges, root first;
 * n_nodes_out_dev int32[n_sel] or NULL.  max_tree_nodes: the node capacity of one tree (root included), 1 .. 2048; every device
 * loop is bounded by it.
 * DRLGX_E_INVALID: a bad argument or algorithm, an environment that does not exist, a non-zero safe_distance or the Dubins control
 * model (drlgx_set_sampler_parameter; the opt-ins drlgx_set_sampler_obstacles and drlgx_set_dubins_leaf_scoring serve them).  DRLGX_E_CAPACITY: a tree needs more than max_tree_nodes nodes, a tree is deeper than
 * max_actions, or a leaf is refused by drlgx_em_cost (more than 256 predicted measurements); the outputs are then unspecified,
 * live state and the status word are untouched, and the remedy is a larger max_tree_nodes or an engine created with a larger
 * max_actions.  The call synchronises twice: once to read the leaf counts and the capacity flag, once in drlgx_em_cost's check. */
int drlgx_em_plan(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *halton_start_dev, int max_tree_nodes,
                  int algorithm, double *plan_out_dev, int32_t *n_actions_out_dev, double *cost_out_dev, int32_t *result_out_dev,
                  int32_t *n_leaves_out_dev, int32_t *halton_next_out_dev, double *nodes_out_dev, int32_t *n_nodes_out_dev);
/* EMPlanner2D::optimize2 under the two occupancy-grid algorithms (Planner2D.cpp:305-319, :1043-1128): drlgx_em_plan's tree - the same
 * kernel, so the same Halton start on the same belief gives the same nodes whatever the algorithm, and the sampler's obstacle logic
 * behind drlgx_set_sampler_obstacles is served in the same way -, drlgx_em_plan's leaves in node order and drlgx_em_plan's pick (the
 * first leaf is always taken - which is also :1106-1108, "the first leaf replaces the root" -, a later one replaces it only on a
 * strictly smaller cost, a NaN never replaces), with the leaf cost of
 *   algorithm DRLGX_ALG_OG_SHANNON: drlgx_og_cost - the same bits as that call on the same leaf.  The leaves of a tree share the
 *     landmarks' cells and the P old poses, so one kernel walks those once per environment and a second one walks each leaf's own
 *     poses from there (k_og.hip: k_og_tree_base, k_og_tree_cost; the development switch DRLGX_OG_TREE_SHARED=0 scores every leaf
 *     with drlgx_og_cost's kernel instead);
 *   algorithm DRLGX_ALG_SLAM_OG_SHANNON: the body of drlgx_slam_og_cost with `alpha` (read under this algorithm only) - the weights
 *     from the live belief, the covariance update in chunks of 128, H_leaf as under algorithm 2; the same bits as that call.  An
 *     environment without a landmark has NaN costs and therefore plans to its first leaf: nothing is special-cased.
 * (The reference cannot run these paths as shipped - Node::map stays a null pointer, see drlgx_og_cost - so the definition is
 * optimize2's control flow as written with the leaf costs above.)  Arrays, max_tree_nodes and result as drlgx_em_plan; live
 * environments are only read.  drlgx_em_plan_leaves reports the scored leaves afterwards.
 * DRLGX_E_INVALID: another algorithm value, alpha outside [0, 1] under algorithm 3, the Dubins flag of drlgx_set_sampler_parameter set
 * (the Dubins control model stays out here, with or without a library: plans of per-step rows cannot be executed yet anyway), and
 * everything drlgx_em_plan refuses as a bad argument.  DRLGX_E_CAPACITY, the outputs then unspecified, live state and the status word
 * untouched: a tree needs more than max_tree_nodes nodes or is deeper than max_actions, or - algorithm 3 - a leaf predicts more than
 * 256 measurements.  Synchronisations: one under algorithm 2 (the tree's leaf counts and capacity flag; its leaves need no further
 * check), two under algorithm 3 (that one and the candidate check of drlgx_slam_og_cost's body). */
int drlgx_og_plan(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *halton_start_dev, int max_tree_nodes,
                  int algorithm, double alpha, double *plan_out_dev, int32_t *n_actions_out_dev, double *cost_out_dev,
                  int32_t *result_out_dev, int32_t *n_leaves_out_dev, int32_t *halton_next_out_dev, double *nodes_out_dev,
                  int32_t *n_nodes_out_dev);
/* EMPlanner2D::rrt_planner (Planner2D.cpp:838-935): the same tree, grown until a new node lies within max_edge_length of the goal
 * (isReached, :88-99: Euclidean distance), to which the goal Pose2(gx, gy, pi) is then connected by connectNode; the plan is the
 * path root -> goal.  The goal of environment i is the position of graph node goal_key[i] if 0 <= goal_key[i] < key_size
 * (landmarks in key order, then poses: the node order of drlgx_graph), else the frontier point goal_xy[i].
 * goal_key_dev int32[n_sel]; goal_xy_dev double[n_sel*2]; the other arrays as above.  A tree that fills max_tree_nodes without
 * reaching its goal reports SAMPLING_FAILURE in result_out_dev with n_actions_out = 0 (the call itself returns DRLGX_OK);
 * DRLGX_E_CAPACITY: a path to a goal longer than max_actions.  One synchronisation (the capacity flag).  Under the Dubins control
 * model (drlgx_set_dubins_library_host) the plan has one row per step and nodes_out columns 5-7 are (library index, num_steps, 0). */
int drlgx_rrt_plan(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *goal_key_dev, const double *goal_xy_dev,
                   const int32_t *halton_start_dev, int max_tree_nodes, double *plan_out_dev, int32_t *n_actions_out_dev,
                   int32_t *result_out_dev, int32_t *halton_next_out_dev, double *nodes_out_dev, int32_t *n_nodes_out_dev);

/* Simulator2D::addLandmarks(landmarks, num_random, params) with a non-empty list (Simulator2D.cpp:445-464; the ini file's
 * optional [Landmarks] section, scripts/envs/pyss2d.py:107-115): the n_fixed listed points take the ground-truth keys
 * 0 .. n_fixed - 1 of EVERY env, the remaining cfg.num_landmarks - n_fixed are sampled as before (cfg.num_landmarks is the
 * total).  HOST array xy [n_fixed][2]; takes effect at the next (staged) reset; n_fixed = 0 restores pure sampling. */
int drlgx_set_fixed_landmarks_host(drlgx_engine *e, int n_fixed, const double *xy);
/* EMPlanner2D(parameter, ...) / EMPlanner2D::setParameter (src/Planner2D.cpp:73-77): the planner constants the kernels
 * read (line-plan edge length, utility weights, occupancy threshold, distance angle weight, algorithm) can be replaced
 * after drlgx_create - the reference constructs its planner after the simulator / SLAM objects. */
int drlgx_set_planner_parameter(drlgx_engine *e, double angle_weight, double distance_weight0, double distance_weight1,
                                double occupancy_threshold, double max_edge_length, int algorithm);

/* EMPlanner2D::calculateUtility (static; src/em_exploration/Planner2D.cpp:354-366) for every
 * environment: U = sum_v tr(info_v^-1) + dist * (w0 - (w0 - w1) * known / V).
 * dist_dev: DEVICE double[n_envs] or NULL (= 0); out_dev: DEVICE double[n_envs]. */
int drlgx_utility(drlgx_engine *e, const double *dist_dev, double *out_dev);
/* EMPlanner2D::calculateUncertainty_EM (Planner2D.cpp:321-341): weighted trace (EM_AOPT) or
 * sum 1[p>0.49]/det(info) (EM_DOPT).  out_dev: DEVICE double[n_envs]. */
int drlgx_uncertainty_em(drlgx_engine *e, int algorithm, double *out_dev);
/* VirtualMap::explored (src/em_exploration/VirtualMap.cpp:47-59). out_dev: DEVICE double[n_envs]. */
int drlgx_explored(drlgx_engine *e, double *out_dev);

/* The metric trio of the reference's evaluation script (scripts/test.py:136-142) for every environment, on the device:
 * out_dev: DEVICE double[n_envs*3] = landmark error (scripts/envs/exploration_env.py:170-177, with its sigma0 argument),
 * map entropy (scripts/test.py:61-74; its per-map-size constant is 0.5 ln 0.5 x the number of padding cells),
 * max localisation uncertainty = max_i tr(marginalCovariance(x_i)) (exploration_env.py:190-194). */
int drlgx_metrics(drlgx_engine *e, double sigma0, double *out_dev);
/* VirtualMap::toCovArray (src/SS2D.cpp:239, src/em_exploration/VirtualMap.cpp:140-151) for every environment:
 * length_dev / angle_dev: DEVICE double[n_envs*rows*cols], row-major grids (min(sqrt(larger eigenvalue of the cell
 * covariance), sigma0) and the direction of its eigenvector). */
int drlgx_cov_array(drlgx_engine *e, double *length_dev, double *angle_dev);

/* ---- planner calls used by the DRL loop ------------------------------------------------------ */

/* EMPlanner2D::line_planner (Planner2D.cpp:937-1041), frontier-goal branch, for n_cand goals.
 * cand_env_dev: DEVICE int32[n_cand]; goal_dev: DEVICE double[n_cand*2];
 * actions_dev: DEVICE double[n_cand*max_actions*3] (x, y, theta); n_actions_dev: DEVICE int32[n_cand]. */
int drlgx_line_plan(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *goal_dev,
                    double *actions_dev, int32_t *n_actions_dev);

/* EMPlanner2D::simulations_reward (Planner2D.cpp:1416-1468) for n_cand candidates
 * (any n_cand >= 0; more than n_rollouts candidates run in successive waves of n_rollouts; n_rollouts must be
 * >= 1): deep-copies the belief and simulator state of env cand_env[i] (including
 * the RNG states), re-solves at the best estimate (SLAM2D::set_copy_isam, SLAM2D.cpp:490-497), rolls
 * the action list forward with one noisy move/measure + SLAM2D::copy_optimize + virtual-map rebuild
 * per action and returns reward = U_before(0) - U_after(dist).  Live environments are not modified.
 * rewards_dev: DEVICE double[n_cand]. */
int drlgx_lookahead(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev,
                    const int32_t *n_actions_dev, double *rewards_dev);

/* drlgx_lookahead with a host-side bound on the plan lengths: max_n_actions >= every n_actions_dev[i] (the caller
 * usually knows it from stepping the chosen plan; 0 < max_n_actions <= max_actions).  Action indices beyond it are
 * not launched at all (drlgx_lookahead launches all max_actions of them and lets the workgroups exit).  Where the fused
 * step kernels serve the pose counts the rollouts reach, a candidate's WHOLE action list runs inside one workgroup (two
 * launches per wave of candidates instead of one per action index) and the rollouts' simulator - whose draws do not depend
 * on the SLAM state - is run ahead for the whole list and replayed; same rewards bit for bit (DRLGX_LOOKAHEAD_LOOP=0 /
 * DRLGX_LOOKAHEAD_PRESIM=0 switch the two off for A/B runs). */
int drlgx_lookahead_bounded(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev,
                            const int32_t *n_actions_dev, int max_n_actions, double *rewards_dev);

/* ---- graph export for the policy (a14-a17) --------------------------------------------------- */

/* ExplorationEnv.frontier + graph_matrix (scripts/envs/exploration_env.py:196-348) on top of
 * SLAM2D::adjacency_degree_get (SLAM2D.cpp:198-273) and DeepQ.data_process (scripts/policy.py:211-232),
 * batched: one graph per environment, concatenated PyG-Batch style.
 *   node order per graph: landmarks by ground-truth key, poses by index, frontier nodes.
 * Outputs (DEVICE, caller-sized with the capacities from drlgx_graph_capacity):
 *   node_off[n_envs+1], edge_off[n_envs+1]      int32 prefix offsets
 *   x[total_nodes*5] float32                    features (trace, dist, bearing diff, prob, type)
 *   edge_index[2*total_edges] int64             (row array then col array, global node ids)
 *   edge_attr[total_edges] float32
 *   n_frontier[n_envs] int32, frontier_xy[n_envs*max_frontier*2] double
 *   nearest_frontier_node[n_envs] int32         local node id of the robot's nearest frontier
 * Edge order inside a graph is DeepQ.data_process's (row-major first-seen, both directions). */
int drlgx_graph_capacity(const drlgx_engine *e, int *max_nodes, int *max_edges, int *max_frontier);
int drlgx_graph(drlgx_engine *e, int32_t *node_off_dev, int32_t *edge_off_dev, float *x_dev,
                int64_t *edge_index_dev, float *edge_attr_dev, int32_t *n_frontier_dev, double *frontier_xy_dev,
                int32_t *nearest_frontier_node_dev);

/* ---- state export (getters of the pybind surface; HOST outputs, synchronise) ------------------ */

/* counts per instance: out[0]=poses, out[1]=landmarks, out[2]=factors, out[3]=step, out[4]=isam update count */
int drlgx_get_counts_host(drlgx_engine *e, int inst, int32_t out[5]);
/* the same five counts for every live env, asynchronously on the engine stream: counts_dev[n_envs*5] (device).
 * Replaces the per-env Python reads `slam.key_size()`, `slam.map.get_landmark_size()`, `sim.step` in a batched loop. */
int drlgx_counts(drlgx_engine *e, int32_t *counts_dev);
/* Environment.iter_trajectory / get_current_vehicle of SLAM2D.map (src/SS2D.cpp:141-171):
 * xytheta[P*3], information[P*9] (may be NULL). */
int drlgx_get_poses_host(drlgx_engine *e, int inst, double *xytheta, double *information);
/* Environment.iter_landmarks of SLAM2D.map, sorted by ground-truth key: keys[L], xy[L*2], information[L*4]. */
int drlgx_get_landmarks_host(drlgx_engine *e, int inst, int32_t *keys, double *xy, double *information);
/* marginal-covariance traces (SLAM2D::features_out, SLAM2D.h:74-76): landmarks by key, then poses. */
int drlgx_get_cov_traces_host(drlgx_engine *e, int inst, double *lm_trace, double *pose_trace);
/* VirtualMap.to_array / to_cov_trace / iter_virtual_landmarks (src/SS2D.cpp:226-246):
 * prob[V], info[V*4] (2x2 row-major), cov_trace[V], updated[V]; any may be NULL. rows/cols via drlgx_vm_shape. */
int drlgx_vm_shape(const drlgx_engine *e, int *rows, int *cols);
int drlgx_get_virtual_map_host(drlgx_engine *e, int inst, double *prob, double *info, double *cov_trace,
                               uint8_t *updated);
/* Simulator2D.vehicle / Simulator2D.environment (ground truth): vehicle_xytheta[3], landmarks_xy[num*2] by key. */
int drlgx_get_ground_truth_host(drlgx_engine *e, int inst, double *vehicle_xytheta, double *landmarks_xy);
/* SLAM2D::adjacency_out / features_out (dense, (L+P)^2 and L+P doubles) for one environment. */
int drlgx_get_adjacency_host(drlgx_engine *e, int inst, double *adjacency, double *features);
/* factor list: pose index, landmark key, bearing, range (M each). */
int drlgx_get_factors_host(drlgx_engine *e, int inst, int32_t *pose, int32_t *key, double *bearing, double *range);
/* libstdc++ iteration order of the ground-truth landmark hash map (Simulator2D.cpp:331-344): order[num]. */
int drlgx_get_landmark_order_host(const drlgx_engine *e, int32_t *order);

/* Snapshot / restore of live environments (device-to-device; used by benchmarks and by
 * ExplorationEnv-style "copy" semantics).  slot in [0, n_snapshots) — allocated lazily. */
int drlgx_snapshot(drlgx_engine *e, int slot);
int drlgx_restore(drlgx_engine *e, int slot);

/* Per-kernel timing (HIP events on the engine stream): enable (on = 1: spans around whatever is launched; on = 2: the
 * belief step is launched as its three stage kernels instead of the fused kernel, so that each stage gets its own span),
 * then read accumulated milliseconds and launch counts.  timer ids: 0 sim, 1 slam, 2 map, 3 copy/prepare, 4 graph,
 * 5 fused belief step (sim + slam + map), 6 the leaf scoring of drlgx_og_plan (the entropy kernels), 7 = an EMPTY span recorded once per drlgx_step (the event-pair overhead a caller
 * subtracts from the per-launch averages).  */
#define DRLGX_N_TIMERS 8
int drlgx_timing_enable(drlgx_engine *e, int on);
int drlgx_timing_read_host(drlgx_engine *e, double ms[DRLGX_N_TIMERS], int64_t launches[DRLGX_N_TIMERS]);

/* Development aid: in-kernel phase stamps (wall_clock64, 100 MHz) of ONE workgroup of the belief kernels.  arm = 0 disarms;
 * arm & 1 arms; arm >> 8 = the workgroup (instance index inside the launch) that stamps, 0 by default.  Slots: 0-7 the SLAM
 * back end, 8-13 the simulator, 14 / 24-35 the SLAM front end, 16-21 / 40-43 / 48-63 the map stage.  out (may be NULL)
 * receives the last stamps: 64 values - the first bank; with arm & 2 the second bank (per-wave cycle stamps of one block
 * step of the sweep); with arm & 4 all 1024 values (out must hold them): both banks and, from 128 on, the start / end stamp
 * of every workgroup of the last k_step launch (scripts/phase_profile*.py). */
int drlgx_debug_phase_clocks_host(drlgx_engine *e, int arm, int64_t *out /* 64 values; 1024 with arm & 4 (read from the buffer's start) */);

/* Development aid: the tile of C per workgroup the GCN's fp32 GEMM dispatcher picks for an m x n product computed in k_slices
 * K-slices (transpose_a: A is stored [K x M], the weight-gradient products), as 1000 * columns + rows: 64064 = the 64x64
 * kernels, 128096..128160 / 64096..64160 = the tall-tile kernel k_gemm_wide with 8 / 4 waves (csrc/k_gemm.hip).  The numerics
 * tests use it to prove that they cover every compiled tile. */
int drlgx_debug_gemm_tile_rows(int m, int n, int k_slices, int transpose_a);

/* Development aid: picks the form of the stand-alone virtual-map kernel (VirtualMap::updateProbability / updateInformation,
 * VirtualMap.cpp:61-84,256-316) for every later launch of this process: 1 = the two-workgroups-per-CU form, 0 = the
 * resident form, -1 (the default; the environment variable DRLGX_MAP_COMPACT sets the initial value, read once) = by launch
 * size: two per CU when there are more instances than CUs.  Returns the previous value.  Both forms are bit-equal; the
 * parity test switches between them with this call. */
int drlgx_debug_map_form(int form);

/* Development aid: 1 when the two-workgroups-per-CU form can serve this engine at a launch bound of p_bound poses, 0 when every
 * map launch runs the resident form whatever drlgx_debug_map_form asks for: a sensor whose bounding box prunes, a carve beyond
 * half the LDS, or a sensor disc that can hold more cell centres than the compact stage has room for per pose (40; the host
 * bounds the lattice count - 41 at a radius of 3.5 cells, the 8-cell window). */
int drlgx_debug_map_compact_ok(const drlgx_engine *e, int p_bound);

/* Development aid, stateless and host-only: the bound drlgx_create puts on the cell centres within max_range of a pose
 * (radius_cells = max_range / resolution, 0 .. 64), so that a CPU test can hold it against a brute-force lattice count. */
int drlgx_debug_disc_cells_bound(double radius_cells);

/* Development aid, stateless and host-only: the code paths the pose-chain solver (csrc/k_slam_arrow.hip) takes for a full solve
 * of an instance with P poses, L landmarks and M factors in an engine whose max_landmarks is L_max - its LDS carve
 * (csrc/arrow_carve.h) at the kernel instantiation and the LDS request drlgx_launch_slam uses, and the predicates of its pose
 * products; mk_panel: the solve leaves a covariance panel (the incremental update is on).  out[DRLGX_ARROW_FORM_N]:
 *   [0] landmark system: 0 packed in LDS, 1 register tiles over the workspace, 2 streamed
 *   [1] obs_lds  [2] xs_lds  [3] rec_lds: observation table / separator rows / factor records in LDS (1) or workspace (0)
 *   [4] form of the pose products: 0 vector units, 1 register-panel tiles, 2 staged
 *   [5] zfit: column tiles of operand images the LDS holds (staged form; 0: the images lie in the streamed sweep's panels)
 *   [6] zg: column tiles per group (staged form)   [7] Tn: tile rows of the landmark system   [8] nK: K chunks of a product
 * A CPU test proves with it that a world lands in the cell it claims.  Returns DRLGX_E_INVALID for counts out of range
 * (P < 1, L < 0, M < 0, L > L_max) and for a landmark system this engine's kernel does not serve. */
#define DRLGX_ARROW_FORM_N 9
int drlgx_debug_arrow_form(int P, int L, int M, int L_max, int mk_panel, int32_t out[DRLGX_ARROW_FORM_N]);

/* Development aid, stateless and host-only: the form the incremental (rank-k) belief update (csrc/k_inc.hip: inc_plan, inc_post)
 * chooses for the update that brings an instance to P poses, with L0 landmarks in its covariance panel and n_re of them
 * re-observed - the LDS plan of csrc/inc_carve.h, the header the kernel takes its plan from, evaluated on the host.
 *   pc         the launch's pose bound (drlgx_step: the largest pose count any env can have after the step, at most max_poses)
 *   P_max, L_max, LG   max_poses, max_landmarks and max(num_landmarks, 1) of the engine;   lds_bytes   the launch's dynamic LDS (163840)
 * out[DRLGX_INC_FORM_N]:
 *   [0] feasible: 0 = the fixed part of the plan misses the LDS, the update is a full solve (everything else is then 0)
 *   [1] lds_panel: the panel is staged in LDS (1) or updated in place in HBM / L2 (0)
 *   [2] wide: the second half of Y fits, batches of up to 16 re-observed landmarks (1), or of up to 8 (0)
 *   [3] snt: factor tiles (of 8 landmarks) per walk the streamed form affords, 1 .. 4 (0: no streamed form - the panel in LDS, or
 *       an update of at most 53 poses, which the dense solver's kernels serve)
 *   [4] streamed: this update takes the streamed form (snt > 0 and more landmarks than one batch, or a Y image beyond 512 KB)
 *   [5] the number of walks (streamed) or batches (otherwise) over the panel, 0 .. 8
 *   [6 ..] per walk or batch, its tiles of 8 landmarks: 1 .. snt (streamed); 1 = a narrow batch, 2 = a wide one (otherwise)
 * A test holds its own statement of the form against it, and proves that a world lands in the form it claims.  Returns
 * DRLGX_E_INVALID for counts out of range (P < 2, P > P_max, L0 > L_max, n_re > L0 or > 64, pc > P_max, lds_bytes > 163840). */
#define DRLGX_INC_FORM_N 14
int drlgx_debug_inc_form(int P, int L0, int n_re, int pc, int P_max, int L_max, int LG, int lds_bytes, int32_t out[DRLGX_INC_FORM_N]);

/* The incremental belief update (csrc/k_inc.hip): between relinearisations of the iSAM2 policy (SLAM2D.cpp:10-12: every
 * 10th update, |delta| >= 0.1) SLAM2D::optimize (SLAM2D.cpp:374-430) only gains the new pose's odometry factor and the
 * step's bearing-range factors, so the engine applies the covariance-form update of FastMarginals2::propagate / update
 * (FastMarginals.cpp:188-321) to a per-instance covariance panel instead of re-solving; updates that relinearise, re-based
 * look-ahead copies (SLAM2D::set_copy_isam, SLAM2D.cpp:490-497) and anything the panel cannot serve take the full solve.
 * On by default; DRLGX_INCREMENTAL=0 in the environment of drlgx_create disables it (every update a full solve), as does a
 * panel memory need beyond DRLGX_INC_MAX_GB (default 32).  out[0] = updates served by the rank-k path, out[1] = full
 * solves, since creation or the last call with reset != 0; both -1 when the path is disabled. */
int drlgx_inc_stats_host(drlgx_engine *e, int64_t out[2], int reset);
/* Development aid: the covariance panel of instance `inst` (an env, a look-ahead copy or a snapshot instance).  meta[4] = {valid, P,
 * L, M}; when valid == 1 and panel != NULL, panel receives the live extent, (3 P + 2 L) rows x (3 + 2 L) columns, row-major (pose
 * rows first); panel_cap: doubles the buffer holds.  Like every getter it first settles what a lazy restore owes. */
int drlgx_debug_panel_host(drlgx_engine *e, int inst, int32_t meta[4], double *panel, size_t panel_cap);

/* The compact restore (csrc/k_misc.hip: k_restore_compact): a lazy drlgx_restore by one workgroup per environment over a table of
 * the entries it copies.  On by default; DRLGX_RESTORE_COMPACT=0 in the environment of drlgx_create selects the generic
 * instance-copy kernel (both are bit-equal), as does DRLGX_RESTORE_EAGER=1.
 * Development aid: the table.  info[4] = {entries, how many of them (the first) are moved as 16-byte items - the others as 4-byte
 * words, 1 when drlgx_restore launches the compact kernel, items a workgroup moves per trip of its loop (threads x loads in
 * flight, the 16-byte kind)}; rows (may be NULL; rows_cap: entries it holds) receives per entry {bytes per instance, unit (0 whole
 * slice, 1 / 2 / 3 per pose / landmark / factor, 4 per pose of a valid covariance panel), bytes per unit, sub-slice bytes or 0}. */
int drlgx_debug_restore_table_host(const drlgx_engine *e, int32_t info[4], int64_t *rows, int rows_cap);
/* Development aid, stateless and host-only: the bytes of a table entry's slice an instance copy moves when the source instance
 * counts `count` of the entry's unit (the formula every copy kernel uses), so that a CPU test can hold it against its own. */
int64_t drlgx_debug_field_live_bytes(int64_t stride, int unit, int unit_bytes, int pad, int count);

/* ---- GCN policy (scripts/Networks.py:12-70 over PyG GCNConv(improved=True)) ------------------- */

/* Forward of GCN / PolicyGCN trunk: H1 = relu(Â X W1 + b1), H2 = relu(Â H1 W2 + b2) [* dropout mask],
 * out = H2 Wf^T + bf, with Â = D^-1/2 (A_w + 2I) D^-1/2 built from (edge_index, edge_attr).
 * All pointers DEVICE, fp32 (edge_index int64 as PyG).  hidden = W1 cols, out_dim = Wf rows.
 * ws_dev: workspace of drlgx_gcn_workspace_bytes(); it keeps what the backward call needs (AX, b1, AH1, H2, both CSRs). */
size_t drlgx_gcn_workspace_bytes(int n_nodes, int n_edges, int hidden, int out_dim);
int drlgx_gcn_forward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim,
                      const float *x, const int64_t *edge_index, const float *edge_attr, const float *W1,
                      const float *b1, const float *W2, const float *b2, const float *Wf, const float *bf,
                      const float *dropout_mask /* [n_nodes*hidden] or NULL */, float *out /* [n_nodes*out_dim] */,
                      void *ws_dev);
/* The same forward for a BATCH of graphs whose boundaries the caller knows (a PyG `Batch` / what drlgx_graph and
 * drlgx_replay_collate emit): graph g owns nodes [node_off[g], node_off[g+1]) and edges [edge_off[g], edge_off[g+1]),
 * DEVICE int32 [n_graphs + 1]; every edge connects two nodes of its own graph (others are ignored); no graph has more
 * than max_edges_per_graph edges (a host-side bound the caller knows: the export's capacity, the collation's counts).
 * Same results bit for bit; the graph normalisation / CSR build is one launch (one workgroup per graph, its edges
 * sorted in LDS) instead of eight; bounds beyond 16 384 edges per graph take the generic build. */
int drlgx_gcn_forward_batched(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim,
                              const float *x, const int64_t *edge_index, const float *edge_attr, const float *W1,
                              const float *b1, const float *W2, const float *b2, const float *Wf, const float *bf,
                              const float *dropout_mask, float *out, void *ws_dev, int n_graphs,
                              const int32_t *node_off, const int32_t *edge_off, int max_edges_per_graph);
/* Backward: given d(out) returns gradients of all six parameter tensors (accumulated = overwritten). */
int drlgx_gcn_backward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim,
                       const float *x, const int64_t *edge_index, const float *edge_attr, const float *W1,
                       const float *W2, const float *Wf, const float *dropout_mask, const float *d_out,
                       float *dW1, float *db1, float *dW2, float *db2, float *dWf, float *dbf, void *ws_dev);

/* ---- GG-NN policy (scripts/Networks.py:73-122 over PyG 1.x GatedGraphConv(1000, 3)) ------------ */

/* Forward of the GGNN / PolicyGGNN / ValueGGNN trunk (scripts/Networks.py:73-122): h_0 = [x | 0] (in_dim <= 8 columns, zero-padded
 * to hidden); n_layers times  a = (A h) weight[l],  h = GRUCell(a, h)  with (A h)[i] = the sum over the edges e into i
 * (edge_index[1][e] = i) of edge_attr[e] h[edge_index[0][e]] - raw weights, no self loops added, no normalisation - and the GRU
 * cell of torch.nn.GRUCell (w_ih / w_hh [3 hidden][hidden], b_ih / b_hh [3 hidden], gate order r, z, n); then
 * out = (relu(h) [* dropout mask]) Wf^T + bf.  All pointers DEVICE, fp32 (edge_index int64 as PyG); weight, b_ih, b_hh and
 * the mask 16-byte aligned.  n_graphs > 0: the batch's graph boundaries as drlgx_gcn_forward_batched takes them (both CSRs in one
 * launch while no graph has more than 2 048 edges); n_graphs <= 0: the generic CSR build.  Same results bit for bit.
 * Edges: repeated edges add up; an edge with an endpoint outside [0, n_nodes) is ignored, with graph boundaries also one whose
 * endpoints are not both in the graph that owns its slot (the generic build keeps an in-range edge between two graphs: give it
 * none); an explicit self loop (i, i) is the node's self weight, of which there is ONE per node: of two self loops on one node
 * only one counts, and which is not defined (both builds).
 * ws_dev: workspace of drlgx_ggnn_workspace_bytes(); it keeps what the backward call needs (both CSRs and per layer h, A h,
 * a and the gates r, z, n, W_hn h + b_hn).  DRLGX_E_INVALID: in_dim > 8, in_dim > hidden, hidden & 3, n_layers < 1 (or > 16),
 * null pointers. */
size_t drlgx_ggnn_workspace_bytes(int n_nodes, int n_edges, int hidden, int n_layers, int out_dim);
int drlgx_ggnn_forward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int n_layers, int out_dim,
                       const float *x, const int64_t *edge_index, const float *edge_attr,
                       const float *weight /*[L,h,h]*/, const float *w_ih /*[3h,h]*/, const float *w_hh,
                       const float *b_ih, const float *b_hh, const float *Wf, const float *bf,
                       const float *dropout_mask /* [n_nodes*hidden] or NULL */, float *out, void *ws_dev,
                       int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_edges_per_graph);
/* Backward of the same trunk (scripts/Networks.py:73-122), after drlgx_ggnn_forward on the same workspace: given d(out) writes
 * (not accumulates) the gradients of all seven parameter tensors; rows in_dim.. of d_weight[0] are zeros.  Deterministic. */
int drlgx_ggnn_backward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int n_layers, int out_dim,
                        const float *x, const int64_t *edge_index, const float *edge_attr, const float *weight,
                        const float *w_ih, const float *w_hh, const float *Wf, const float *dropout_mask, const float *d_out,
                        float *d_weight, float *d_w_ih, float *d_w_hh, float *d_b_ih, float *d_b_hh,
                        float *dWf, float *dbf, void *ws_dev);

/* ---- g-U-Net policy (scripts/Networks.py:125-449 over PyG 1.x GraphUNet / TopKPooling) --------- */

/* Forward of the GraphUNet / PolicyGraphUNet / ValueGraphUNet trunk with sum_res and relu:
 *   x_0 = relu(conv_d0(x, A_0));  for l = 1..depth:  B = offdiag((A_{l-1} + I)^2),  s = tanh(x_{l-1} . p_l / |p_l|),  perm_l = per
 *   graph the k = ceil(pool_ratio n_g) nodes of largest s (equal scores: the lower node index; kept nodes stay in ascending index,
 *   so pooled batches stay grouped by graph),  A_l = B[perm_l, perm_l] relabelled,  x_l = relu(conv_dl(x_{l-1}[perm_l] s[perm_l], A_l));
 *   for i = 0..depth-1, j = depth-1-i:  x = relu(conv_ui(x_j + up, A_j)), up[perm_{j+1}] = x (the last relu is the trunk's own and
 *   carries the dropout mask);  out = x Wf^T + bf.
 * M[edge_index[0][e], edge_index[1][e]] = edge_attr[e], duplicates sum, (M M)[i][j] = sum_k M[i][k] M[k][j]; the added self loops
 * weigh 1; B keeps every structurally non-zero off-diagonal entry.  Every conv is GCNConv(improved=True) as drlgx_gcn_forward
 * computes it.  Edge weights are data: no gradient.  ceil is taken of the double product.
 * params: HOST array of 5 depth + 4 DEVICE pointers in state_dict order - down_convs.{0..depth}.{weight [in][hidden], bias},
 * pools.{0..depth-1}.weight [hidden], up_convs.{0..depth-1}.{weight [hidden][hidden], bias}, fully_con1.{weight [out_dim][hidden],
 * bias} - all fp32 and 16-byte aligned, as the mask.  Graph boundaries as drlgx_gcn_forward_batched takes them (DEVICE int32
 * [n_graphs + 1]; edges of graph g in [edge_off[g], edge_off[g+1]), an edge that leaves its graph is ignored); n_graphs = 0: the
 * whole input is one graph.  max_graph_nodes: a HOST bound on the nodes of one graph (at most 4 096: the augment keeps dense
 * rows of a graph in LDS).
 * ws_dev: workspace of drlgx_unet_workspace_bytes() for the same sizes, ws_bytes its size; it keeps what the backward call
 * needs (per level both CSRs, the pooled edge list, scores, kept sets, the convs' aggregated inputs and relu outputs).
 * The levels' sizes are read back from the device once per call (the call synchronises the stream).
 * DRLGX_E_INVALID: in_dim > 8, hidden & 3, depth outside 1..4, pool_ratio outside (0, 1], null or misaligned pointers, node_off
 * that does not end at n_nodes.  DRLGX_E_CAPACITY: ws_bytes too small (nothing is written), a graph larger than max_graph_nodes
 * or than 4 096 nodes (only the level offsets have been written). */
size_t drlgx_unet_workspace_bytes(int n_nodes, int n_edges, int n_graphs, int max_graph_nodes, int hidden, int depth, double pool_ratio,
                                  int out_dim);
int drlgx_unet_forward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int depth, double pool_ratio, int out_dim,
                       const float *x, const int64_t *edge_index, const float *edge_attr, const float *const *params,
                       const float *dropout_mask /* [n_nodes*hidden] or NULL */, float *out, void *ws_dev, size_t ws_bytes,
                       int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_graph_nodes);
/* Backward of the same trunk, after drlgx_unet_forward on the same workspace with the same sizes: given d(out) writes (not
 * accumulates) the gradients of all 5 depth + 4 parameter tensors into grads (HOST array of DEVICE pointers, params' order and
 * shapes), d p_l with the term through |p_l|.  Deterministic. */
int drlgx_unet_backward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int depth, double pool_ratio, int out_dim,
                        const float *x, const int64_t *edge_index, const float *edge_attr, const float *const *params,
                        const float *dropout_mask, const float *d_out, float *const *grads, void *ws_dev, size_t ws_bytes,
                        int n_graphs, int max_graph_nodes);
/* The nodes a forward kept at `level` (1..depth), from its workspace: ids of level - 1's nodes, ascending per graph, into perm_out
 * (DEVICE int32, room for n_nodes); *count_host receives their number.  Same sizes as the forward call.  Synchronises. */
int drlgx_unet_kept_nodes(void *hip_stream, int n_nodes, int n_edges, int hidden, int depth, double pool_ratio, int out_dim, void *ws_dev,
                          size_t ws_bytes, int n_graphs, int max_graph_nodes, int level, int32_t *perm_out, int *count_host);
/* The selection alone: per graph the k = ceil(pool_ratio n_g) nodes of largest score, equal scores to the lower index, written
 * in ascending node index.  Out (DEVICE int32): pooled_node_off [n_graphs + 1], pooled_edge_off [n_graphs + 1] or NULL (the
 * prefix of k_g (k_g - 1): where drlgx_unet_augment_filter puts each graph's entries), perm [sum of k_g] (node ids),
 * inverse [n_nodes] or NULL (pooled id of a node, -1 if dropped).  No sort, no atomics: deterministic. */
int drlgx_unet_topk(void *hip_stream, int n_nodes, int n_graphs, const int32_t *node_off, const float *scores, double pool_ratio,
                    int32_t *pooled_node_off, int32_t *pooled_edge_off, int32_t *perm, int32_t *inverse);
/* Augment and filter alone: per graph offdiag((A + I)^2) restricted to the kept nodes `perm` (ascending per graph, as
 * drlgx_unet_topk writes them) and relabelled to pooled ids.  Graph g's entries go to pooled_edge_index [2][pooled_capacity]
 * (int64) / pooled_edge_attr from slot pooled_edge_off[g] on, sorted by (row, column), each (row, column) once; the unused
 * slots up to pooled_edge_off[g+1] get -1 / 0 (the GCN's CSR builders ignore them); pooled_edge_count [n_graphs] (or NULL)
 * receives the entries per graph.  A graph's slot range must hold k_g (k_g - 1) entries; what does not fit is not written.
 * DRLGX_E_CAPACITY: max_graph_nodes > 4 096. */
int drlgx_unet_augment_filter(void *hip_stream, int n_nodes, int n_edges, const int64_t *edge_index, const float *edge_attr, int n_graphs,
                              const int32_t *node_off, const int32_t *edge_off, int max_graph_nodes, const int32_t *perm,
                              const int32_t *pooled_node_off, const int32_t *pooled_edge_off, int64_t pooled_capacity,
                              int64_t *pooled_edge_index, float *pooled_edge_attr, int32_t *pooled_edge_count);

/* ---- DQN update (scripts/policy.py:137-178, :234-253): the pieces between the two GCN calls ---------------- */

/* Mini-batch collation of replay graphs held in a device pool = torch_geometric DataLoader(s_j_batch, batch_size=BATCH)
 * (scripts/policy.py:146-153): graph g is rows [node_start, +node_cnt) of pool_x ([rows][in_dim] f32) and columns
 * [edge_start, +edge_cnt) of pool_ei ([2][pool_edges] i64) / pool_ea, its node ids start at loc.  desc_dev int64
 * [5][n_graphs] = node_start, node_cnt, edge_start, edge_cnt, loc.  Outputs (DEVICE, sized by the caller from the counts):
 * x_out [N][in_dim], ei_out [2][n_edges_total] (ids shifted by the cumulative node counts), ea_out, batch_out [N], and the
 * graph boundaries in the form drlgx_gcn_forward_batched takes.  pool_q / q_out (optional): one float per pooled node
 * gathered the same way - the target network's read-out, which depends on the graph and the (frozen) target weights only and
 * is therefore evaluated once per stored graph and target refresh instead of once per mini-batch (scripts/policy.py:154-156);
 * with x_out NULL only this value is gathered. */
int drlgx_replay_collate(void *hip_stream, int n_graphs, const int64_t *desc_dev, const float *pool_x, int in_dim,
                         const int64_t *pool_ei, int64_t pool_edges, const float *pool_ea, float *x_out, int64_t *ei_out,
                         int64_t n_edges_total, float *ea_out, int64_t *batch_out,
                         int32_t *node_off_out /* [n_graphs + 1] or NULL */, int32_t *edge_off_out /* [n_graphs + 1] or NULL */,
                         const float *pool_q /* [rows] or NULL */, float *q_out /* [N] or NULL */);
/* The two collations of one DQN mini-batch in one launch (scripts/policy.py:146-156): the current states s_j as
 * drlgx_replay_collate emits them, and - for the next states s_j1, desc2_dev int64 [5][n_graphs] - only the cached per-node
 * value pool_q gathered into q2_out [sum of their node counts] (the target network's read-out over the collated s_j1). */
int drlgx_replay_collate_pair(void *hip_stream, int n_graphs, const int64_t *desc_dev, const float *pool_x, int in_dim,
                              const int64_t *pool_ei, int64_t pool_edges, const float *pool_ea, float *x_out, int64_t *ei_out,
                              int64_t n_edges_total, float *ea_out, int64_t *batch_out, int32_t *node_off_out, int32_t *edge_off_out,
                              const int64_t *desc2_dev, const float *pool_q, float *q2_out);
/* TD targets, scripts/policy.py:154-175: sample i takes max(q1[lo_i:hi_i]) (float32, the target network's read-out over
 * the collated next states; the caller resolves the reference's slicing into [lo, hi)), and
 * a_batch[pos_i] = 1, y_batch[pos_i] = r_i + gamma max  (r_i alone when terminal_i) in float64; both vectors
 * [n_nodes_total] are zeroed first.  meta_dev int64 [4][n_samples] = lo, hi, pos, terminal; r_dev double [n_samples]. */
int drlgx_dqn_targets(void *hip_stream, int n_samples, const float *q1, const int64_t *meta_dev, const double *r_dev,
                      double gamma, int64_t n_nodes_total, double *a_batch, double *y_batch);
/* DeepQ.cost (scripts/policy.py:234-239) and d(cost)/d(pred): loss_out[0] = sum (pred a - y)^2 / batch (float64),
 * d_pred float32 [n_nodes] - what loss.backward() hands to the network (scripts/policy.py:249). */
int drlgx_dqn_loss_grad(void *hip_stream, int n_nodes, const float *pred, const double *action, const double *y,
                        double batch, double *loss_out, float *d_pred);
/* `param.grad.data.clamp_(-c, c)` + torch.optim.Adam.step() (scripts/policy.py:250-253; lr as given, no weight decay /
 * amsgrad) for up to 8 fp32 tensors in one launch.  HOST arrays of DEVICE pointers; step = 1 for the first update;
 * grad_clamp <= 0 disables the clamp. */
int drlgx_adam_step(void *hip_stream, int n_tensors, float *const *params, const float *const *grads,
                    float *const *exp_avg, float *const *exp_avg_sq, const int64_t *sizes, double lr, double beta1,
                    double beta2, double eps, int64_t step, double grad_clamp);
/* ... with the gradient multiplied by grad_scale in front of the clamp: the 1 / world-size of a SUM all-reduced gradient
 * (scripts/policy.py has one process; the build's data-parallel trainer averages over ranks - SURVEY.md 8e) folded in. */
int drlgx_adam_step_scaled(void *hip_stream, int n_tensors, float *const *params, const float *const *grads,
                    float *const *exp_avg, float *const *exp_avg_sq, const int64_t *sizes, double lr, double beta1,
                    double beta2, double eps, int64_t step, double grad_clamp, double grad_scale);

/* Replay graphs never change once stored, so what drlgx_gcn_forward_batched derives from a graph - weighted degrees, self
 * weights, both CSRs with the normalised weights D^-1/2 (A_w + 2I) D^-1/2 (GCNConv(improved=True), scripts/Networks.py:15-16)
 * and Â X - is computed ONCE per stored export and kept beside the pooled graphs, graph-local (row starts / ends relative to
 * the graph's first edge, neighbour ids to its first node).  DEVICE arrays over the pool's node rows / edge columns. */
typedef struct drlgx_csr_cache {
  float *deg, *selfw, *ax;                         /* [nodes], [nodes], [nodes][8] */
  int32_t *ptr_dst, *end_dst, *ptr_src, *end_src;  /* [nodes] */
  int32_t *nbr_dst, *nbr_src;                      /* [edges] */
  float *wn_dst, *wn_src;                          /* [edges] */
} drlgx_csr_cache;
/* Fill the cache for one export of n_graphs graphs (boundaries node_off / edge_off, DEVICE int32 [n_graphs + 1], relative to
 * the export's first node / edge).  x, edge_index (second row at + edge_row_stride), edge_attr and every array of `cache`
 * point AT the export's first node / edge.  DRLGX_E_CAPACITY: a graph has more edges than the per-graph kernel sorts
 * (16 384) - the caller keeps that export uncached and collates it the generic way. */
int drlgx_replay_cache_csr(void *hip_stream, int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_edges_per_graph,
                           const float *x, int in_dim, const int64_t *edge_index, int64_t edge_row_stride, const float *edge_attr,
                           const drlgx_csr_cache *cache);
/* Mini-batch collation straight into the graph part of a GCN workspace (ws_dev of drlgx_gcn_workspace_bytes(n_nodes,
 * n_edges, ...)): the cached arrays of graph g (desc_dev as drlgx_replay_collate; `cache` points at the POOL's first node /
 * edge) land at its cumulative offsets with row bounds / neighbour ids shifted - bit for bit what
 * drlgx_gcn_forward_batched builds for the collated batch.  desc2_dev / pool_q / q2_out: as drlgx_replay_collate_pair
 * (or all NULL).  Then drlgx_gcn_forward_prebuilt runs the forward without touching x / edge_index / edge_attr. */
int drlgx_gcn_collate_csr(void *hip_stream, int n_graphs, const int64_t *desc_dev, const drlgx_csr_cache *cache, int n_nodes,
                          int n_edges, int hidden, int out_dim, void *ws_dev, int32_t *node_off_out, int32_t *edge_off_out,
                          const int64_t *desc2_dev, const float *pool_q, float *q2_out);
int drlgx_gcn_forward_prebuilt(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim, const float *W1,
                               const float *b1, const float *W2, const float *b2, const float *Wf, const float *bf,
                               const float *dropout_mask, float *out, void *ws_dev);

/* One DQN update as TWO host calls (scripts/policy.py:139-178 and :234-249).  Nothing new runs on the device - the launches of
 * drlgx_replay_collate_pair + drlgx_dqn_targets (prepare), and of drlgx_gcn_forward_batched + drlgx_dqn_loss_grad +
 * drlgx_gcn_backward (forward_backward), are issued back to back on the caller's stream with every intermediate in ONE
 * caller-owned DEVICE arena of drlgx_dqn_arena_bytes(): the 256-env trainer was bound by the host work of those launches.
 * The arena's layout is a function of the capacities (cap_nodes / cap_edges of the collated current states, cap_nodes1 of the
 * next states' read-out) only; both calls of an update - and drlgx_dqn_arena_views, for read-backs - must pass the same ones.
 * views[12] = x, edge_index [2][n_edges], edge_attr, batch, node_off, edge_off, q1, a_batch, y_batch, out, d_out, loss.
 * params / grads: HOST arrays of six DEVICE pointers (W1 b1 W2 b2 Wf bf and their gradients, written not accumulated).
 * cache (or NULL): the pool's drlgx_csr_cache - prepare then collates the cached graph data straight into the GCN workspace
 * (drlgx_gcn_collate_csr) instead of x / edge_index / edge_attr, and forward_backward (same `cache`-ness) skips the build. */
size_t drlgx_dqn_arena_bytes(int n_graphs, int64_t cap_nodes, int64_t cap_edges, int64_t cap_nodes1, int in_dim, int hidden,
                             int out_dim);
int drlgx_dqn_arena_views(void *arena_dev, int n_graphs, int64_t cap_nodes, int64_t cap_edges, int64_t cap_nodes1, int in_dim,
                          int hidden, int out_dim, void **views);
int drlgx_dqn_prepare(void *hip_stream, int n_graphs, const int64_t *desc_dev, const int64_t *desc1_dev, const float *pool_x,
                      int in_dim, const int64_t *pool_ei, int64_t pool_edges, const float *pool_ea, const float *pool_q,
                      int64_t n_nodes, int64_t n_edges, int64_t n_nodes1, const int64_t *meta_dev, const double *r_dev,
                      double gamma, void *arena_dev, int64_t cap_nodes, int64_t cap_edges, int64_t cap_nodes1, int hidden,
                      int out_dim, const drlgx_csr_cache *cache);
int drlgx_dqn_forward_backward(void *hip_stream, int n_graphs, int64_t n_nodes, int64_t n_edges, int max_edges_per_graph,
                               int in_dim, int hidden, int out_dim, const float *const *params, const float *dropout_mask,
                               double batch, float *const *grads, void *arena_dev, int64_t cap_nodes, int64_t cap_edges,
                               int64_t cap_nodes1, int graph_prebuilt);

/* ---- env wrapper / actor-critic heads ------------------------------------------------------------------------- */

/* The normalisation of ExplorationEnv.rewards_all_goals (scripts/envs/exploration_env.py:151-161) for every env: raw
 * look-ahead rewards of env e's frontiers at [cand_first[e], +n_frontier[e]) -> np.interp onto [-1, 0] (nearest frontier
 * is the first arg-max, loop_clo 0) or [-1, 1] (loop_clo 1).  All pointers DEVICE. */
int drlgx_normalise_rewards(void *hip_stream, int n_envs, const double *raw, const int64_t *cand_first,
                            const int32_t *n_frontier, double *out, uint8_t *loop_clo);
/* PolicyGCN head (scripts/Networks.py:47-50): masked_select + torch_geometric.utils.softmax over every graph's selected
 * nodes.  q / mask over all N nodes, graph boundaries node_off int32 [n_graphs + 1]; p_out holds the selected nodes of
 * all graphs in node order (sum(mask) values).  Backward: d_q over all N nodes (0 outside the mask). */
int drlgx_segment_softmax(void *hip_stream, int n_graphs, const int32_t *node_off, const float *q, const uint8_t *mask,
                          float *p_out);
int drlgx_segment_softmax_backward(void *hip_stream, int n_graphs, const int32_t *node_off, const float *p,
                                   const float *d_p, const uint8_t *mask, float *d_q);
/* ValueGCN head (scripts/Networks.py:66-70): global_mean_pool(h, batch).mean(dim=1) of the [N][n_cols] read-out, one
 * value per graph; backward d_h [N][n_cols]. */
int drlgx_mean_pool(void *hip_stream, int n_graphs, const int32_t *node_off, const float *h, int n_cols, float *v_out);
int drlgx_mean_pool_backward(void *hip_stream, int n_graphs, const int32_t *node_off, const float *d_v, int n_cols,
                             float *d_h);

/* ---- evaluation driver --------------------------------------------------------------------------------------------- */

/* The greedy decision of the reference's evaluation loop (scripts/test.py:110-119) for every env, on the device, one wave per
 * env: choice[e] = np.argmax(score[seg_begin[e] : seg_begin[e] + n_frontier[e]]) - the first maximum, a NaN before every number,
 * the first NaN - and the line plan to that frontier slot out of the padded plans drlgx_line_plan emits over all
 * n_envs x max_frontier slots: actions_out[e] = actions_pad[e][choice[e]] with the actions beyond n_act_pad[e][choice[e]]
 * written as zeros, n_actions_out[e] = that length.  An env with active[e] == 0 (active_dev NULL = all active) or without
 * frontiers gets choice -1, n_actions_out 0 and a zero plan.  score: float32 [n_score], covering every segment (for DQN the
 * per-node read-out with seg_begin = node_off[e + 1] - n_frontier[e], for A2C the compact soft-max output with seg_begin = the
 * exclusive prefix sum of n_frontier).  actions_pad double [n_envs][max_frontier][max_actions][3], n_act_pad int32
 * [n_envs][max_frontier], actions_out double [n_envs][max_actions][3].  All pointers DEVICE. */
int drlgx_greedy_plans(void *hip_stream, int n_envs, const float *score, int n_score, const int32_t *seg_begin, const int32_t *n_frontier,
                       const uint8_t *active_dev, const double *actions_pad, const int32_t *n_act_pad, int max_frontier,
                       int max_actions, int32_t *choice, double *actions_out, int32_t *n_actions_out);

#ifdef __cplusplus
}
#endif
#endif /* DRLGX_H */
