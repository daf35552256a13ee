// drlgx engine: host side of the C ABI (include/drlgx.h) — HBM state allocation, kernel
// orchestration for reset / step / look-ahead, state export.  No CPU compute path exists here: every
// belief-step quantity is produced by the HIP kernels in k_*.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <cstdlib>
#include <vector>

#include "drlgx_dev.h"
#include "drlgx_fields.h"
#include "fm2_carve.h"

#define HIPCHK(e, call)                                                                       \
  do {                                                                                        \
    hipError_t _r = (call);                                                                   \
    if (_r != hipSuccess) {                                                                   \
      (e)->last_error = std::string(#call) + ": " + hipGetErrorString(_r);                    \
      return DRLGX_E_HIP;                                                                     \
    }                                                                                         \
  } while (0)

struct TimedSpan {
  hipEvent_t a, b;
  int id;
};

struct drlgx_engine {
  DrlgxState S{};
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::vector<void *> allocs;
  // the state struct's copy in device memory (DrlgxState::self_dev) and what was uploaded last: every entry point compares and
  // re-uploads before it launches anything (state_sync), whatever changed the struct
  DrlgxState *state_dev = nullptr;
  unsigned char state_shadow[sizeof(DrlgxState)];
  std::vector<DrlgxField> fields;       // per-instance fields (n_inst instances)
  DrlgxField *fields_dev = nullptr;
  // the compact restore's table (drlgx_restore_table): the first restore_n16 entries are moved as 16-byte items
  std::vector<DrlgxField> restore_tab;
  DrlgxField *restore_tab_dev = nullptr;
  int restore_n16 = 0;
  std::vector<int> lm_order;
  // staging
  int32_t *stage_i32 = nullptr;
  uint32_t *stage_u32 = nullptr;
  double *stage_f64 = nullptr;
  uint8_t *stage_mask = nullptr;
  int *graph_gi = nullptr;
  int graph_gi_stride = 0;
  // timing
  bool timing = false;
  // Host-side upper bound of every env's pose count: exact after drlgx_reset_host / drlgx_status_host / a restore of a
  // snapshot taken in an exact state, +1 per drlgx_step in between (the active mask lives on the device).  It selects
  // the k_slam variant and whether the fused step kernel applies, per launch, so that a large pose capacity does not
  // slow the steps of short trajectories down.
  std::vector<int> pbound;
  bool by_capacity = false;  // DRLGX_VARIANT_BY_CAPACITY=1 (tests): select the variants by max_poses as if every env were full
  std::vector<std::vector<int>> snap_pbound;
  bool per_stage = false;  // timing mode 2: launch the three stage kernels separately so that each gets its own span
  std::vector<TimedSpan> spans;
  std::vector<hipEvent_t> free_events;
  double t_ms[DRLGX_N_TIMERS] = {0};
  int64_t t_n[DRLGX_N_TIMERS] = {0};
  std::string last_error;
  double *fixed_lm_dev = nullptr;  // drlgx_set_fixed_landmarks_host
  unsigned char *simlog_dev = nullptr;  // the look-ahead's simulator log (k_presim), n_rollouts x max_actions entries
  bool la_presim = true;
  // drlgx_status_host / drlgx_status_fetch_host wait by polling an event (DRLGX_SYNC_SPIN=0: hipStreamSynchronize): a trainer's vector
  // step reads the status word four times, each on the critical path between two launches, and a blocking wait hands the thread
  // back tens of microseconds after the stream drained
  bool spin_sync = true;
  hipEvent_t sync_event = nullptr;
  // packed status reads (k_fetch_pack): device staging and its pinned host mirror, grown on demand
  unsigned char *fetch_dev = nullptr, *fetch_host = nullptr;
  size_t fetch_cap = 0;
  int n_cu = 256;       // compute units of the device (drlgx_create)
  bool la_loop = true;  // look-ahead rollouts: one launch for a candidate's whole action list (k_step_loop)
  // FastMarginals2 workspaces (allocated on first use): dense prior covariances, per-candidate scratch
  double *fm2_sig = nullptr, *fm2_scratch = nullptr;
  int *fm2_iscratch = nullptr;
  size_t fm2_sig_stride = 0;
  // drlgx_em_cost (allocated on first use): the covariances and pose counts of one chunk of candidates
  double *em_cov = nullptr;
  int32_t *em_nout = nullptr;
  int *check_flag = nullptr;  // the argument checks' flag word (run_check; allocated on first use)
  // drlgx_slam_og_cost (allocated on first use / grown on demand): the root weights [n_envs][2], one chunk's landmark blocks
  // [kFm2Chunk][L_max][3]; per candidate the leaf entropy [cap] and the cost's distance factors [cap][2]
  double *sog_weights = nullptr, *sog_lm = nullptr, *sog_h = nullptr, *sog_dist = nullptr;
  size_t sog_cap = 0;
  // drlgx_og_plan (allocated on first use): what the leaves of a tree share - per environment the ladder state of every cell after
  // the landmarks and the old poses [n_envs][Vu], and the known cells of the live map [n_envs] (k_og_tree_base).
  // DRLGX_OG_TREE_SHARED=0: the leaves are scored by k_og_cost, each from the untouched map (the A/B of the shared base)
  uint8_t *og_base = nullptr;
  int32_t *og_known = nullptr;
  bool og_tree_shared = true;
  // drlgx_em_plan / drlgx_rrt_plan (grown on demand): the trees' tables (edge odometry, parent and depth, leaf list, per-tree
  // results), the leaves as candidates of drlgx_em_cost with their costs; the sampler's own planner parameters
  double *tree_act = nullptr, *tree_cand_act = nullptr, *tree_cost = nullptr;
  int *tree_link = nullptr, *tree_leaf = nullptr, *tree_meta = nullptr;
  int32_t *tree_cand_env = nullptr, *tree_cand_n = nullptr;
  size_t tree_nodes_cap = 0, tree_sel_cap = 0, tree_cand_cap = 0;
  double sampler_max_nodes = 0.5, sampler_safe_distance = 0.0;
  int sampler_dubins = 0;
  int sampler_obstacles = 0;  // drlgx_set_sampler_obstacles: the sampler's obstacle logic (safe_distance > 0), off unless asked for
  // drlgx_set_env_obstacles: SS2D.simulate's obstacle flag at cfg.safe_distance > 0, off unless asked for; drlgx_follow_plans'
  // selected actions [n_envs][max_actions][3] (allocated on first use)
  int env_obstacles = 0;
  double *follow_act = nullptr;
  // drlgx_set_dubins_leaf_scoring: drlgx_em_plan under the Dubins control model, off unless asked for; the leaves' core masks and
  // tree distances (grown with the candidates), the number of candidates the last served call left (drlgx_em_plan_leaves)
  int dubins_leaf_scoring = 0;
  uint8_t *tree_cand_core = nullptr;
  double *tree_cand_dist = nullptr;
  size_t tree_cand_steps_cap = 0, tree_cand_last = 0;
  bool tree_cand_last_steps = false;
  // drlgx_set_dubins_library_host: the Dubins path library, the opt-in of the Dubins control model (dubins.n == 0: none loaded) - on
  // the device for the kernel, on the host for drlgx_dubins_library; the nodes' poses for the plan (grown with the trees' tables)
  DrlgxDubins dubins = {};
  double *dub_end_x = nullptr, *dub_end_y = nullptr, *dub_v = nullptr, *dub_w = nullptr, *tree_pose = nullptr;
  int *dub_steps = nullptr;
  size_t dub_cap = 0, tree_pose_cap = 0;
  double dub_reach = 0.0;
  int dub_prefilter = 1;
  std::vector<double> dub_end_h, dub_v_h, dub_w_h;  // end: x y theta per entry
  std::vector<int> dub_steps_h;
  // Lazy restore: drlgx_restore leaves the virtual-map planes (field class 1) in the snapshot - the next belief step rebuilds
  // every cell of them without reading them (LaunchSel::vm_from) - and the bodies of the valid covariance panels, which that step
  // reads there and stores into the env (kPanelInSrc in the panel's header); it records the slot here (-1: every env holds its own).
  // Any other entry point settles the debt first (settle: one copy of planes and bodies).  DRLGX_RESTORE_EAGER=1: the full copy.
  int owed_slot = -1;
  bool restore_eager = false;
  // DRLGX_RESTORE_COMPACT=0: a lazy restore runs the generic copy kernel, not k_restore_compact (the A/B of the compact restore)
  bool restore_compact = true;
};

// every entry point makes the engine's device current (a process may drive several engines on several devices) and - all but
// those that neither read nor write instance state, and drlgx_restore / drlgx_step themselves (DRLGX_ENTER_OWING) - settles
// what a lazy restore still owes, so that no entry point can see an env without its planes
#define DRLGX_ENTER_OWING(e)                    \
  do {                                          \
    if (e) {                                    \
      (void)hipSetDevice((e)->device);          \
      state_sync(e);                            \
    }                                           \
  } while (0)
#define DRLGX_ENTER(e)                          \
  do {                                          \
    DRLGX_ENTER_OWING(e);                       \
    if (e) settle(e);                           \
  } while (0)

struct drlgx_engine;
static void state_sync(drlgx_engine *e);
static void settle(drlgx_engine *e);

namespace {

template <typename T>
int dev_alloc(drlgx_engine *e, T **out, size_t count) {
  void *p = nullptr;
  size_t bytes = std::max<size_t>(count * sizeof(T), 256);
  HIPCHK(e, hipMalloc(&p, bytes));
  HIPCHK(e, hipMemsetAsync(p, 0, bytes, e->stream));
  e->allocs.push_back(p);
  *out = reinterpret_cast<T *>(p);
  return DRLGX_OK;
}

template <typename T>
int field_alloc(drlgx_engine *e, T **out, size_t per_inst, int cls = 0, int unit = 0, size_t per_unit = 0) {
  int r = dev_alloc(e, out, per_inst * (size_t)e->S.n_inst);
  if (r) return r;
  e->fields.push_back(DrlgxField{reinterpret_cast<char *>(*out), per_inst * sizeof(T), cls, unit, (int)(per_unit * sizeof(T)), 0});
  return DRLGX_OK;
}

hipEvent_t get_event(drlgx_engine *e) {
  if (!e->free_events.empty()) {
    hipEvent_t ev = e->free_events.back();
    e->free_events.pop_back();
    return ev;
  }
  hipEvent_t ev;
  hipEventCreate(&ev);
  return ev;
}
struct ScopedTimer {
  drlgx_engine *e;
  TimedSpan s;
  bool on;
  ScopedTimer(drlgx_engine *e_, int id) : e(e_), on(e_->timing) {
    if (on) {
      s.a = get_event(e);
      s.b = get_event(e);
      s.id = id;
      hipEventRecord(s.a, e->stream);
    }
  }
  ~ScopedTimer() {
    if (on) {
      hipEventRecord(s.b, e->stream);
      e->spans.push_back(s);
    }
  }
};

int check_launch(drlgx_engine *e) {
  hipError_t r = hipGetLastError();
  if (r != hipSuccess) {
    e->last_error = std::string("kernel launch: ") + hipGetErrorString(r);
    return DRLGX_E_HIP;
  }
  return DRLGX_OK;
}

}  // namespace

// ---- drlgx_create in parts: each returns an error code, drlgx_create destroys the half-built engine on any of them ----------
#define TRY(x)             \
  do {                     \
    int r_ = (x);          \
    if (r_) return r_;     \
  } while (0)

// why the last drlgx_create of this thread failed: what drlgx_last_error(NULL) returns, no engine being left to ask
static thread_local std::string g_create_error;

static int check_config(const drlgx_config *cfg, int n_envs, int n_rollouts) {
  if (!cfg || n_envs <= 0 || n_rollouts < 0) return DRLGX_E_INVALID;
  if (cfg->max_poses < 2 || cfg->max_landmarks < 1 || cfg->max_factors < 1 || cfg->num_landmarks < 0 ||
      cfg->max_actions < 1 || cfg->num_samples < 1)
    return DRLGX_E_INVALID;
  // the interior cell count divides by (int)resolution, as VirtualMap.cpp:341 does (set_map_constants): a resolution below 1
  // (NaN included) is a division by zero there
  if (!(cfg->resolution >= 1)) {
    g_create_error = "resolution must be at least 1";
    return DRLGX_E_INVALID;
  }
  // kernel limits: 16-bit pose / landmark / factor indices in LDS tables; the per-pose / per-landmark tables of k_slam_arrow
  // must fit the LDS (its landmark system is streamed from the workspace beyond 127 landmarks)
  if (cfg->max_poses > 65535 || cfg->max_landmarks > 65535 || cfg->max_factors > 65534) return DRLGX_E_INVALID;
  if (!drlgx_slam_capacity_ok(cfg->max_poses, cfg->max_landmarks, cfg->max_factors)) return DRLGX_E_INVALID;
  // the graph export keeps a frontier table per cell and an observation table per (landmark, pose) pair in LDS (k_graph.hip);
  // drlgx_slam_capacity_ok does not bound that product (500 landmarks x 200 poses pass it and need 200 KB there)
  const double cells = std::floor((cfg->map_max_x - cfg->map_min_x) / cfg->resolution) *
                       std::floor((cfg->map_max_y - cfg->map_min_y) / cfg->resolution);  // (set_map_constants: S.V; it refuses V <= 0)
  if (!(cells <= 65535.0) || !drlgx_graph_capacity_ok(cfg->max_poses, cfg->max_landmarks, (int)cells)) {
    g_create_error = "max_landmarks x max_poses (or the cell count of the map) too large for the LDS tables of the graph export";
    return DRLGX_E_INVALID;
  }
  // the map kernel keeps its per-pose tables, two masks and a landmark count per cell in LDS (kmap::MapCarve); with one pose per
  // pass it takes the least it can
  if (kmap::MapCarve(cfg->max_poses, 1, (int)cells, false).bytes > kmap::kLdsBudget) {
    g_create_error = "map too large for the LDS tables of the map kernel";
    return DRLGX_E_INVALID;
  }
  // the simulator kernels keep a measure() call's variates and its in-range list in LDS, per listed landmark (k_sim.hip); their
  // launches set no LDS attribute, so kSimLdsLimit bounds them: k_reset and the step's simulator stage for every engine, k_presim
  // (one measure() per action) for one with look-ahead rollouts.  The obstacle opt-in has its own, lower bound (sim_obs_fits).
  const int LG = std::max(cfg->num_landmarks, 1);
  if (drlgx_sim_launch_lds(DRLGX_SIM_RESET, LG) > kSimLdsLimit || drlgx_sim_launch_lds(DRLGX_SIM_STEP, LG) > kSimLdsLimit ||
      drlgx_sim_launch_lds(DRLGX_SIM_STAGE, LG) > kSimLdsLimit ||
      (n_rollouts > 0 && drlgx_sim_launch_lds(DRLGX_SIM_PRESIM, LG, 1) > kSimLdsLimit)) {
    g_create_error = "num_landmarks too large for the LDS of the simulator kernels (k_reset / k_sim_step / k_presim)";
    return DRLGX_E_INVALID;
  }
  return DRLGX_OK;
}

// a switch of the environment: its first character decides ('0' turns a default-on switch off, '1' a default-off one on)
static bool env_flag(const char *name, bool dflt) {
  const char *v = getenv(name);
  if (!v) return dflt;
  return dflt ? v[0] != '0' : v[0] == '1';
}

static void read_env_switches(drlgx_engine *e) {
  e->by_capacity = env_flag("DRLGX_VARIANT_BY_CAPACITY", false);
  e->spin_sync = env_flag("DRLGX_SYNC_SPIN", true);
  e->la_presim = env_flag("DRLGX_LOOKAHEAD_PRESIM", true);  // 0: every rollout action simulates inside its belief step (the A/B of the parity test)
  e->la_loop = env_flag("DRLGX_LOOKAHEAD_LOOP", true);  // 0: one launch per action index (the A/B of the look-ahead tests)
  e->restore_eager = env_flag("DRLGX_RESTORE_EAGER", false);  // 1: a restore copies the virtual-map planes and panel bodies too (the A/B of the lazy restore)
  e->restore_compact = env_flag("DRLGX_RESTORE_COMPACT", true);  // 0: a lazy restore by the generic copy kernel (the A/B of the compact restore)
  e->og_tree_shared = env_flag("DRLGX_OG_TREE_SHARED", true);  // 0: drlgx_og_plan scores its leaves with k_og_cost (the A/B of the shared base)
}

static double p2l(double p) { return std::log(p / (1.0 - p)); }
static double l2p(double l) { return std::exp(l) / (1.0 + std::exp(l)); }

// Upper bound on the lattice points an open disc of radius r (in cells) holds, wherever its centre lies.  By the lattice's
// symmetries the centre may be taken in [0, 1/2]^2; that square is covered by 32 x 32 sub-squares of side h = 1 / 64, every centre lies
// within h / sqrt(2) of the middle of one, so the disc around it lies inside the disc of radius r + h / sqrt(2) around that middle:
// the largest count over the 1024 middles bounds every centre's.  (3.0 cells, the default sensor at resolution 2: 32, the true
// maximum; 3.5 cells: 41 - reached 0.2 to 0.35 cell off a lattice point along one axis.)
static int disc_cells_bound(double r) {
  const int n = 32;
  const double h = 0.5 / n, rr = r + h * 0.70710678118654752440 + 1e-9;
  const int k = (int)std::ceil(rr) + 1;
  int best = 0;
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      const double u = (a + 0.5) * h, v = (b + 0.5) * h;
      int cnt = 0;
      for (int i = -k; i <= k; ++i)
        for (int j = -k; j <= k; ++j)
          if ((i - u) * (i - u) + (j - v) * (j - v) <= rr * rr) ++cnt;
      best = std::max(best, cnt);
    }
  return best;
}

// capacities, map geometry and the log-odds / noise constants
static int set_map_constants(drlgx_engine *e) {
  DrlgxState &S = e->S;
  const drlgx_config *cfg = &S.cfg;
  S.P_max = cfg->max_poses;
  S.L_max = cfg->max_landmarks;
  S.M_max = cfg->max_factors;
  S.LG = std::max(cfg->num_landmarks, 1);
  S.A_max = cfg->max_actions;
  // VirtualMap::initialize (VirtualMap.cpp:318-343)
  S.cols = (int)std::floor((cfg->map_max_x - cfg->map_min_x) / cfg->resolution);
  S.rows = (int)std::floor((cfg->map_max_y - cfg->map_min_y) / cfg->resolution);
  S.V = S.rows * S.cols;
  S.Vu = (S.V + 3) / 4 * 4;
  {
    int extg = 20;
    S.count_explored = (S.rows - extg * 2 / (int)cfg->resolution) * (S.cols - extg * 2 / (int)cfg->resolution);
  }
  // OccupancyMap uses ceil() for its grid (OccupancyMap.cpp:13-14); the reference asserts equal sizes
  if ((int)std::ceil((cfg->map_max_x - cfg->map_min_x) / cfg->resolution) != S.cols ||
      (int)std::ceil((cfg->map_max_y - cfg->map_min_y) / cfg->resolution) != S.rows || S.V <= 0) {
    e->last_error = "map extent must be a multiple of the resolution";
    return DRLGX_E_INVALID;
  }
  S.win = (int)std::ceil(2.0 * cfg->max_range / cfg->resolution) + 1;
  if (S.win * S.win > 64) {
    e->last_error = "max_range / resolution too large for the 64-lane cell window";
    return DRLGX_E_INVALID;
  }
  // in-range cells per pose (the map kernel's compact form has room for kmap::kPairsPerPose of them: map_lds_bytes_compact)
  S.disc_cells = disc_cells_bound(cfg->max_range / cfg->resolution);
  // log-odds constants (OccupancyMap.h:10-19) evaluated with the HOST libm: exact ladder values
  S.lo_free = p2l(0.3);
  S.lo_occ = p2l(0.7);
  S.lo_min = p2l(0.05);
  S.lo_max = l2p(0.95);  // sic: MAX_LOGODDS = LOGODDS2PROB(0.95)
  S.occ_thresh = p2l(0.5);
  S.vm_i0 = 1.0 / std::pow(cfg->sigma0, 2);
  S.w_trans = 1.0 / (cfg->translation_noise * cfg->translation_noise);
  S.w_rot = 1.0 / (cfg->rotation_noise * cfg->rotation_noise);
  S.w_bear = 1.0 / (cfg->bearing_noise * cfg->bearing_noise);
  S.w_range = 1.0 / (cfg->range_noise * cfg->range_noise);
  return DRLGX_OK;
}

// occupancy ladder closure (see DrlgxState::lo_tocc): the packed transition tables into S, the value table for the upload
static int build_ladder(drlgx_engine *e, std::vector<double> &lo_pv) {
  DrlgxState &S = e->S;
  const drlgx_config *cfg = &S.cfg;
  std::vector<uint8_t> lo_tr;  // per state: next on occupied, next on free, flags (1: at the minimum - frozen, 2: above the threshold)
  S.lo_tocc = S.lo_tfree = 0ull;
  S.lo_tflag = 0u;
  std::vector<double> lo_val{0.0};
  auto clampl = [&](double l) { return std::fmin(S.lo_max, std::fmax(S.lo_min, l)); };
  auto find_or_add = [&](double l) -> int {
    for (size_t i = 0; i < lo_val.size(); ++i)
      if (lo_val[i] == l) return (int)i;
    lo_val.push_back(l);
    return (int)lo_val.size() - 1;
  };
  // Only the transitions the update rules can take are followed (OccupancyMap.cpp:55-138): the landmark pre-updates
  // apply `occupied` along the chain 0 -> occ(0) -> ...; a pose update leaves a cell at the minimum alone, adds
  // `occupied` above the threshold and `free` otherwise.  (Following both successors of every state does not close:
  // lo_occ and lo_free are not exact negatives of each other in floating point, so the values drift by ulps.)
  bool closed = true;
  std::vector<int> is_chain{1};  // states reachable by landmark pre-updates alone
  for (size_t i = 0; i < lo_val.size(); ++i) {
    if (lo_val.size() > DRLGX_LO_TAB) {
      closed = false;
      break;
    }
    const double l = lo_val[i];
    const bool frozen = std::fabs(l - S.lo_min) < 1e-5, above = l > S.occ_thresh + 1e-8;
    int o = (int)i, f = (int)i;
    if (above || is_chain[i]) {
      o = find_or_add(clampl(l + S.lo_occ));
      if ((size_t)o >= is_chain.size()) is_chain.push_back(0);
      if (is_chain[i]) is_chain[o] = 1;
    }
    if (!above && !frozen) {
      f = find_or_add(clampl(l + S.lo_free));
      if ((size_t)f >= is_chain.size()) is_chain.push_back(0);
    }
    const uint8_t flags = (uint8_t)((frozen ? 1 : 0) | (above ? 2 : 0));
    lo_tr.push_back((uint8_t)o); lo_tr.push_back((uint8_t)f); lo_tr.push_back(flags);
  }
  // The kernels walk the packed tables and have no other form of the ladder.  The log-odds constants are not configuration
  // (set_map_constants fixes them), and with them the closure always ends on the same six states - 0, 0.7211, -0.8473, -1.6946,
  // -2.5419, -2.9444; num_samples only changes lo_pv - so this cannot happen unless those constants change.
  if (!closed || lo_val.size() > DRLGX_LO_TAB) {
    e->last_error = "occupancy ladder does not close within 16 states";
    return DRLGX_E_INVALID;
  }
  for (double l : lo_val) {  // OccupancyMap LOGODDS2PROB + VirtualMap::updateProbability (num_samples identical maps)
    const double pv1 = l2p(l);
    double acc = 0.0;
    for (int s2 = 0; s2 < cfg->num_samples; ++s2) acc += pv1 / cfg->num_samples;
    lo_pv.push_back(acc);
  }
  S.lo_ntab = (int)lo_val.size();
  for (int i = 0; i < S.lo_ntab; ++i) {
    S.lo_tocc |= (unsigned long long)(lo_tr[3 * i] & 15) << (4 * i);
    S.lo_tfree |= (unsigned long long)(lo_tr[3 * i + 1] & 15) << (4 * i);
    S.lo_tflag |= (unsigned int)(lo_tr[3 * i + 2] & 3) << (2 * i);
  }
  return DRLGX_OK;
}

// sector-sweep table (OccupancyMap.cpp:86) and what follows from the sensor's sector and range: bbox_noop, fov_*, r2_*
static std::vector<double> set_sensor_constants(DrlgxState &S) {
  const drlgx_config *cfg = &S.cfg;
  // b accumulates in double exactly as the reference loop
  std::vector<double> sweep;
  for (double b = cfg->min_bearing; b < cfg->max_bearing + 1e-5; b += 3 * 0.01745329251994329575) sweep.push_back(b);
  S.n_sweep = (int)sweep.size();
  // The bbox only prunes work if an in-range cell can fall outside it.  A cell centre within max_range of the
  // pose lies at most (max_range - res/2) past the pose's own cell boundary, so the box contains it as soon as
  // some sweep sample is within acos(1 - res / (2 max_range)) of each axis direction (k_map).
  const double two_pi = 6.283185307179586476925286766559;
  double max_gap = 3 * 0.01745329251994329575;
  if (!sweep.empty()) max_gap = std::max(max_gap, two_pi - (sweep.back() - sweep.front()));
  const double need = std::acos(std::max(-1.0, 1.0 - cfg->resolution / (2.0 * cfg->max_range)));
  S.bbox_noop = (0.5 * max_gap + 1e-6 <= need) ? 1 : 0;
  // field of view: blind half-angle around the backwards ray
  const double pi = 3.14159265358979323846;
  const double blind = std::max(pi - cfg->max_bearing, pi + cfg->min_bearing);
  S.fov_fast = (cfg->max_bearing > 1.7 && cfg->min_bearing < -1.7 && blind >= 0 && blind + 1e-3 < 1.4) ? 1 : 0;
  S.fov_tan = S.fov_fast ? std::tan(blind + 1e-3) : 0.0;
  // smallest x with sqrt(x) >= max_range, largest x with sqrt(x) <= min_range (sqrt is correctly rounded
  // and monotone on both host and device, so the squared comparisons are EXACTLY the reference's tests)
  double t = cfg->max_range * cfg->max_range;
  while (std::sqrt(std::nextafter(t, 0.0)) >= cfg->max_range) t = std::nextafter(t, 0.0);
  while (std::sqrt(t) < cfg->max_range) t = std::nextafter(t, INFINITY);
  S.r2_max_lt = t;
  t = cfg->min_range * cfg->min_range;
  while (std::sqrt(std::nextafter(t, INFINITY)) <= cfg->min_range) t = std::nextafter(t, INFINITY);
  while (t > 0 && std::sqrt(t) > cfg->min_range) t = std::nextafter(t, 0.0);
  S.r2_min_gt = t;
  return sweep;
}

template <typename T>
static int upload_table(drlgx_engine *e, const T **out, const std::vector<T> &host) {
  T *dev = nullptr;
  TRY(dev_alloc(e, &dev, host.size()));
  HIPCHK(e, hipMemcpyAsync(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, e->stream));
  *out = dev;
  return DRLGX_OK;
}

// the per-instance fields, in the order the copy table is built from (drlgx_create sorts it stably afterwards)
static int alloc_fields(drlgx_engine *e) {
  DrlgxState &S = e->S;
  const size_t P = S.P_max, L = S.L_max, M = S.M_max, V = S.V;
  TRY(field_alloc(e, &S.gt_pose, 4));
  TRY(field_alloc(e, &S.parent, 1));
  TRY(field_alloc(e, &S.mt, 2 * DRLGX_MT_STRIDE));
  TRY(field_alloc(e, &S.nrm_saved, 2));
  TRY(field_alloc(e, &S.nrm_has, 2));
  TRY(field_alloc(e, &S.cnt, DRLGX_CNT_STRIDE));
  TRY(field_alloc(e, &S.th_pose, P * 4, 0, 1, 4));
  TRY(field_alloc(e, &S.d_pose, P * 3, 0, 1, 3));
  TRY(field_alloc(e, &S.th_lm, L * 2, 0, 2, 2));
  TRY(field_alloc(e, &S.d_lm, L * 2, 0, 2, 2));
  TRY(field_alloc(e, &S.lm_key, L, 0, 2, 1));
  TRY(field_alloc(e, &S.key_slot, (size_t)S.LG));
  TRY(field_alloc(e, &S.prior, DRLGX_PRIOR_STRIDE));
  TRY(field_alloc(e, &S.odo, P * 4, 0, 1, 4));
  TRY(field_alloc(e, &S.meas_pose, M, 0, 3, 1));
  TRY(field_alloc(e, &S.meas_lm, M, 0, 3, 1));
  TRY(field_alloc(e, &S.meas_br, M * 2, 0, 3, 2));
  TRY(field_alloc(e, &S.est_pose, P * 4, 0, 1, 4));
  TRY(field_alloc(e, &S.est_lm, L * 2, 0, 2, 2));
  TRY(field_alloc(e, &S.pose_info, P * 6, 0, 1, 6));
  TRY(field_alloc(e, &S.lm_info, L * 3, 0, 2, 3));
  TRY(field_alloc(e, &S.pose_tr, P, 0, 1, 1));
  TRY(field_alloc(e, &S.lm_tr, L, 0, 2, 1));
  TRY(field_alloc(e, &S.red, DRLGX_RED_STRIDE));
  TRY(field_alloc(e, &S.vm_prob, V, 1));
  TRY(field_alloc(e, &S.vm_info, 3 * V, 1));
  {
    // the three planes of the information as three entries of the copy table (same stride, a third of the bytes each): the 38 KB slice
    // was the copy kernel's longest workgroup by far
    DrlgxField f = e->fields.back();
    e->fields.pop_back();
    for (int k = 0; k < 3; ++k) {
      DrlgxField g = f;
      g.base = f.base + (size_t)k * V * sizeof(double);
      g.pad = (int)(V * sizeof(double));
      e->fields.push_back(g);
    }
  }
  TRY(field_alloc(e, &S.vm_upd, (size_t)S.Vu, 1));
  TRY(field_alloc(e, &S.vm_tr, V, 1));
  TRY(field_alloc(e, &S.gt_lm, (size_t)S.LG * 2, 2));  // rollouts read their parent's landmarks
  return DRLGX_OK;
}

// Covariance panel of the incremental belief update (k_inc.hip): on unless DRLGX_INCREMENTAL=0 or the panels of all
// instances would not fit the budget (DRLGX_INC_MAX_GB; default: 60 % of the memory that is free on the device now) or the
// allocation fails - then every update is a full solve (the engine works either way; said once on stderr).
static int alloc_panels(drlgx_engine *e) {
  DrlgxState &S = e->S;
  const char *g = getenv("DRLGX_INC_MAX_GB");
  size_t free_b = 0, total_b = 0;
  double max_gb = 32.0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) max_gb = 0.6 * (double)free_b / 1073741824.0;
  if (g) max_gb = atof(g);
  S.jc_ld = (3 + 2 * S.L_max + 31) & ~31;  // whole pairs of 16-column tiles, rows on 256-byte boundaries (k_inc.hip, B3)
  S.jc_stride = (size_t)(3 * S.P_max + 2 * S.L_max + 16) * (size_t)S.jc_ld;  // (+ 16: the row tiles are written whole)
  const double gb = (double)S.jc_stride * 8.0 * (double)S.n_inst / 1073741824.0;
  if (!env_flag("DRLGX_INCREMENTAL", true)) return DRLGX_OK;
  const size_t n_before = e->allocs.size();
  bool ok = gb <= max_gb;
  if (ok) {
    ok = dev_alloc(e, &S.jc, S.jc_stride * (size_t)S.n_inst) == DRLGX_OK && dev_alloc(e, &S.jd, (size_t)S.P_max * 6 * (size_t)S.n_inst) == DRLGX_OK &&
         dev_alloc(e, &S.jc_meta, (size_t)4 * (size_t)S.n_inst) == DRLGX_OK && dev_alloc(e, &S.inc_stats, 2) == DRLGX_OK;
  }
  if (!ok) {
    (void)hipGetLastError();  // a failed hipMalloc is not this engine's error
    while (e->allocs.size() > n_before) {
      hipFree(e->allocs.back());
      e->allocs.pop_back();
    }
    S.jc = nullptr;
    S.jd = nullptr;
    S.jc_meta = nullptr;
    S.inc_stats = nullptr;
    e->last_error.clear();
    fprintf(stderr, "drlgx: covariance panels (%.1f GB) not allocated (budget %.1f GB): every belief update is a full solve\n", gb, max_gb);
  }
  return DRLGX_OK;
}

// status word, the copy table, staging buffers and the state struct's device copy
static int alloc_staging(drlgx_engine *e) {
  DrlgxState &S = e->S;
  const int n_envs = S.n_envs;
  TRY(dev_alloc(e, &S.status, 1));
  // (the copy kernel deals a workgroup to every (instance, field): the largest slices first, so that none of them starts last)
  std::stable_sort(e->fields.begin(), e->fields.end(), [](const DrlgxField &a, const DrlgxField &b) {
    return (a.pad > 0 ? (size_t)a.pad : a.stride) > (b.pad > 0 ? (size_t)b.pad : b.stride);
  });
  TRY(dev_alloc(e, &e->fields_dev, e->fields.size()));
  HIPCHK(e, hipMemcpyAsync(e->fields_dev, e->fields.data(), e->fields.size() * sizeof(DrlgxField), hipMemcpyHostToDevice, e->stream));
  e->restore_tab = drlgx_restore_table(e->fields, S.jd, S.P_max, &e->restore_n16);
  TRY(dev_alloc(e, &e->restore_tab_dev, e->restore_tab.size()));
  HIPCHK(e, hipMemcpyAsync(e->restore_tab_dev, e->restore_tab.data(), e->restore_tab.size() * sizeof(DrlgxField), hipMemcpyHostToDevice, e->stream));
  TRY(dev_alloc(e, &e->stage_i32, (size_t)n_envs));
  TRY(dev_alloc(e, &e->stage_u32, (size_t)n_envs));
  TRY(dev_alloc(e, &e->stage_f64, (size_t)n_envs * 3));
  TRY(dev_alloc(e, &e->stage_mask, (size_t)n_envs));
  e->graph_gi_stride = 4 * S.L_max + 8;
  TRY(dev_alloc(e, &e->graph_gi, (size_t)n_envs * e->graph_gi_stride));
  // the struct's device copy: what the belief kernels read their state from (DrlgxStateConst; drlgx_dev.h)
  unsigned char *raw = nullptr;
  TRY(dev_alloc(e, &raw, sizeof(DrlgxState)));
  e->state_dev = reinterpret_cast<DrlgxState *>(raw);
  S.self_dev = e->state_dev;
  return DRLGX_OK;
}

static int build_engine(drlgx_engine *e) {
  DrlgxState &S = e->S;
  const drlgx_config *cfg = &S.cfg;
  if (cfg->max_snapshots < 0 || cfg->max_snapshots > 16) return DRLGX_E_INVALID;
  // instances: [0,n) live envs | [n,2n) look-ahead bases | rollouts | max_snapshots x n snapshot copies
  S.n_inst = 2 * S.n_envs + S.n_roll + cfg->max_snapshots * S.n_envs;
  e->pbound.assign(S.n_envs, cfg->max_poses);  // unknown until the first reset
  e->snap_pbound.assign(cfg->max_snapshots > 0 ? cfg->max_snapshots : 0, std::vector<int>(S.n_envs, cfg->max_poses));
  read_env_switches(e);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, e->device) == hipSuccess && prop.multiProcessorCount > 0) e->n_cu = prop.multiProcessorCount;
  TRY(set_map_constants(e));
  std::vector<double> lo_pv;
  TRY(build_ladder(e, lo_pv));
  const std::vector<double> sweep = set_sensor_constants(S);
  // libstdc++ iteration order of unordered_map<unsigned, ...> filled with keys 0..n-1 (Simulator2D.cpp:331-344)
  {
    std::unordered_map<unsigned, int> m;
    for (int i = 0; i < cfg->num_landmarks; ++i) m.emplace((unsigned)i, i);
    for (const auto &kv : m) e->lm_order.push_back((int)kv.first);
    if (e->lm_order.empty()) e->lm_order.push_back(0);
  }
  TRY(upload_table(e, &S.sweep_b, sweep));
  TRY(upload_table(e, &S.lm_order, e->lm_order));
  TRY(upload_table(e, &S.lo_pv, lo_pv));
  TRY(alloc_fields(e));
  // SLAM workspace (not copied between instances; k_slam_host.hip: drlgx_slam_ws_doubles)
  S.slam_ws_stride = drlgx_slam_ws_doubles(S.P_max, S.L_max, S.M_max);
  S.slam_iws_stride = 2;
  TRY(dev_alloc(e, &S.slam_ws, S.slam_ws_stride * (size_t)S.n_inst));
  TRY(dev_alloc(e, &S.slam_iws, S.slam_iws_stride * (size_t)S.n_inst));
  TRY(alloc_panels(e));
  TRY(alloc_staging(e));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return DRLGX_OK;
}
#undef TRY

extern "C" {

const char *drlgx_strerror(int code) {
  switch (code) {
    case DRLGX_OK: return "ok";
    case DRLGX_E_INVALID: return "invalid argument";
    case DRLGX_E_NODEVICE: return "no HIP device";
    case DRLGX_E_CAPACITY: return "instance capacity exceeded (max_poses / max_landmarks / max_factors / max_actions)";
    case DRLGX_E_HIP: return "HIP runtime error";
    case DRLGX_E_NUMERIC: return "indeterminate linear system in the SLAM solve";
    default: return "unknown error";
  }
}

const char *drlgx_last_error(const drlgx_engine *e) {
  if (e) return e->last_error.c_str();
  return g_create_error.empty() ? "null engine" : g_create_error.c_str();
}

int drlgx_create(const drlgx_config *cfg, int n_envs, int n_rollouts, int device, drlgx_engine **out) {
  if (!out) return DRLGX_E_INVALID;
  g_create_error.clear();
  int r = check_config(cfg, n_envs, n_rollouts);
  if (r) return r;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return DRLGX_E_NODEVICE;
  drlgx_engine *e = new drlgx_engine();
  e->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete e;
    return DRLGX_E_NODEVICE;
  }
  if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete e;
    return DRLGX_E_NODEVICE;
  }
  e->stream = e->own_stream;
  DrlgxState &S = e->S;
  S.cfg = *cfg;
  S.n_envs = n_envs;
  S.n_roll = n_rollouts;
  if ((r = build_engine(e)) != DRLGX_OK) {
    g_create_error = e->last_error;
    drlgx_destroy(e);
    return r;
  }
  state_sync(e);
  *out = e;
  return DRLGX_OK;
}

// The device copy of the state struct follows the host's: compared at every entry point (0.8 KB), uploaded when it differs -
// after whatever the stream still runs with the old one.
static void state_sync(drlgx_engine *e) {
  if (!e->state_dev || memcmp(e->state_shadow, &e->S, sizeof(DrlgxState)) == 0) return;
  (void)hipStreamSynchronize(e->stream);
  (void)hipMemcpy(e->state_dev, &e->S, sizeof(DrlgxState), hipMemcpyHostToDevice);
  memcpy(e->state_shadow, &e->S, sizeof(DrlgxState));
}

// snapshot instance of env 0 in slot `slot`
static int snapshot_base(const drlgx_engine *e, int slot) { return 2 * e->S.n_envs + e->S.n_roll + slot * e->S.n_envs; }

// what a lazy restore still owes: the planes and the marked covariance panel bodies of every env from the restored slot, in one copy
static void settle(drlgx_engine *e) {
  if (e->owed_slot < 0) return;
  drlgx_launch_copy(e->fields_dev, (int)e->fields.size(), e->stream, e->S.n_envs, nullptr, nullptr, snapshot_base(e, e->owed_slot), 0, 0,
                    nullptr, &e->S, 1, 3);
  e->owed_slot = -1;
}

int drlgx_destroy(drlgx_engine *e) {
  DRLGX_ENTER_OWING(e);
  if (!e) return DRLGX_E_INVALID;
  hipDeviceSynchronize();
  for (void *p : e->allocs) hipFree(p);
  for (auto &sp : e->spans) {
    hipEventDestroy(sp.a);
    hipEventDestroy(sp.b);
  }
  for (auto ev : e->free_events) hipEventDestroy(ev);
  if (e->sync_event) hipEventDestroy(e->sync_event);
  if (e->fetch_dev) hipFree(e->fetch_dev);
  if (e->fetch_host) hipHostFree(e->fetch_host);
  if (e->own_stream) hipStreamDestroy(e->own_stream);
  delete e;
  return DRLGX_OK;
}

int drlgx_set_stream(drlgx_engine *e, void *hip_stream) {
  DRLGX_ENTER_OWING(e);  // (callers re-bind before a restore and a step: the debt follows the engine onto the new stream)
  if (!e) return DRLGX_E_INVALID;
  hipStream_t s = (hip_stream == reinterpret_cast<void *>(-1)) ? e->own_stream : reinterpret_cast<hipStream_t>(hip_stream);
  if (s == e->stream) return DRLGX_OK;  // cheap when nothing changes: callers re-bind before every call
  hipStreamSynchronize(e->stream);      // work already queued on the old stream is ordered before the new one's
  e->stream = s;
  return DRLGX_OK;
}

int drlgx_synchronize(drlgx_engine *e) {
  DRLGX_ENTER_OWING(e);
  if (!e) return DRLGX_E_INVALID;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return DRLGX_OK;
}

static int max_bound(const drlgx_engine *e) {
  if (e->by_capacity) return e->S.P_max;
  int m = 1;
  for (int v : e->pbound) m = std::max(m, v);
  return m;
}

// every env may have gained k poses
static void advance_pbound(drlgx_engine *e, int k) {
  for (int &v : e->pbound) v = std::min(v + k, e->S.P_max);
}

// the stream drained, observed by polling (see drlgx_engine::spin_sync)
static hipError_t stream_wait(drlgx_engine *e) {
  if (!e->spin_sync) return hipStreamSynchronize(e->stream);
  if (!e->sync_event && hipEventCreateWithFlags(&e->sync_event, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    e->spin_sync = false;
    return hipStreamSynchronize(e->stream);
  }
  hipError_t r = hipEventRecord(e->sync_event, e->stream);
  if (r != hipSuccess) return r;
  // (polling pays for the waits of a vector step - a look-ahead, a plan execution: up to a few milliseconds; behind a longer queue the
  // thread hands the core back)
  const auto t0 = std::chrono::steady_clock::now();
  for (int polls = 0; (r = hipEventQuery(e->sync_event)) == hipErrorNotReady; ++polls) {
    if ((polls & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(5000)) return hipStreamSynchronize(e->stream);
  }
  return r;
}

// status word + pose counts (+ `bytes` of the caller's device memory -> dst_host) in one launch, one copy and one wait
static int status_fetch(drlgx_engine *e, const void *src_dev, size_t bytes, void *dst_host) {
  const size_t head = drlgx_fetch_head_bytes(e->S.n_envs), total = head + ((bytes + 15) & ~(size_t)15);
  if (total > e->fetch_cap) {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->fetch_dev) (void)hipFree(e->fetch_dev);
    if (e->fetch_host) (void)hipHostFree(e->fetch_host);
    e->fetch_dev = e->fetch_host = nullptr;
    e->fetch_cap = 0;
    const size_t cap = std::max<size_t>(2 * total, 1 << 16);
    HIPCHK(e, hipMalloc(reinterpret_cast<void **>(&e->fetch_dev), cap));
    HIPCHK(e, hipHostMalloc(reinterpret_cast<void **>(&e->fetch_host), cap, hipHostMallocDefault));
    e->fetch_cap = cap;
  }
  drlgx_launch_fetch_pack(e->S, e->stream, src_dev, bytes, e->fetch_dev);
  if (int r = check_launch(e)) return r;
  HIPCHK(e, hipMemcpyAsync(e->fetch_host, e->fetch_dev, head + bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, stream_wait(e));
  const int32_t *h = reinterpret_cast<const int32_t *>(e->fetch_host);
  // the same synchronisation refreshes the host's pose-count bounds with the exact device values
  for (int i = 0; i < e->S.n_envs; ++i) e->pbound[i] = std::min(std::max((int)h[1 + i], 1), e->S.P_max);
  if (bytes) std::memcpy(dst_host, e->fetch_host + head, bytes);
  return h[0];
}

int drlgx_status_host(drlgx_engine *e) {
  DRLGX_ENTER_OWING(e);
  if (!e) return DRLGX_E_INVALID;
  return status_fetch(e, nullptr, 0, nullptr);
}

int drlgx_status_fetch_host(drlgx_engine *e, const void *src_dev, size_t bytes, void *dst_host) {
  DRLGX_ENTER_OWING(e);
  if (!e || (bytes > 0 && (!src_dev || !dst_host))) return DRLGX_E_INVALID;
  // the caller's bytes ride on the status read's synchronisation (a vector step of a trainer needs a handful of small device
  // results on the host: every separate read drains the stream again)
  return status_fetch(e, src_dev, bytes, dst_host);
}

int drlgx_reset_host(drlgx_engine *e, int n, const int32_t *env_ids, const uint32_t *seeds, const double *start) {
  DRLGX_ENTER(e);
  if (!e || n <= 0 || n > e->S.n_envs || !env_ids || !seeds || !start) return DRLGX_E_INVALID;
  std::vector<uint8_t> mask(e->S.n_envs, 0);
  for (int i = 0; i < n; ++i) {
    if (env_ids[i] < 0 || env_ids[i] >= e->S.n_envs || mask[env_ids[i]]) return DRLGX_E_INVALID;
    mask[env_ids[i]] = 1;
  }
  HIPCHK(e, hipMemcpyAsync(e->stage_i32, env_ids, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->stage_u32, seeds, n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->stage_f64, start, n * 3 * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->stage_mask, mask.data(), e->S.n_envs, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemsetAsync(e->S.status, 0, sizeof(int), e->stream));
  drlgx_launch_reset(e->S, e->stream, n, e->stage_i32, e->stage_u32, e->stage_f64);
  for (int i = 0; i < n; ++i) e->pbound[env_ids[i]] = 1;
  LaunchSel sel{0, e->S.n_envs, e->stage_mask, nullptr, 0};
  drlgx_launch_slam(e->S, e->stream, sel, e->by_capacity ? e->S.P_max : 1);
  sel.pcap = max_bound(e);
  drlgx_launch_map(e->S, e->stream, sel, 0);  // reductions only: the virtual map is in its untouched state
  int r = check_launch(e);
  if (r) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));  // staging buffers are reused
  return DRLGX_OK;
}

// One belief step of a selection, in the form its pose bound pb allows: the fused kernel around the dense solver, the same
// fusion around the pose-chain solver (longer trajectories), or the three stage kernels - also in timing mode 2, where each
// stage gets its own span (timers 0-2; the fused forms: timer 5).  n_measure: the simulator's stream selector.
// obstacles: a step of LIVE envs under the obstacle opt-in (env_obstacles_on) - always the three stage kernels, the simulator stage in
// its flag-raising form (k_sim_step_obs); the beliefs are those of the other forms bit for bit (the stage kernels against the fused
// ones: tests/test_gpu_step_edges.py; the flag's simulator against the plain one: tests/test_gpu_obstacle.py).
static void launch_belief_step(drlgx_engine *e, LaunchSel sel, const double *odom, int odom_stride, int n_measure, int pb, bool may_split,
                               bool obstacles = false) {
  const DrlgxState &S = e->S;
  sel.pcap = pb;  // (the kernels size their per-pose LDS tables with the launch's bound, not with the capacity)
  if (drlgx_step_fusable(S, pb) && !e->per_stage && !obstacles) {
    ScopedTimer t(e, 5);
    // more instances than CUs: simulator + SLAM fused, the map as its own launch in the two-workgroups-per-CU form (k_map_c) - at one
    // workgroup per CU the fused map stage cannot overlap anything, two map workgroups per CU cover each other's barriers
    const bool split = may_split && sel.n > e->n_cu && drlgx_map_two_per_cu(S, pb);
    sel.skip_map = split ? 1 : 0;
    drlgx_launch_step(S, e->stream, sel, odom, odom_stride, n_measure);
    if (split) {
      sel.skip_map = 0;
      drlgx_launch_map(S, e->stream, sel, 1);
    }
  } else if (drlgx_step_arrow_fusable(S) && !e->per_stage && !obstacles) {
    ScopedTimer t(e, 5);
    drlgx_launch_step_arrow(S, e->stream, sel, odom, odom_stride, n_measure);
  } else {
    {
      ScopedTimer t(e, 0);
      if (obstacles) drlgx_launch_sim_obs(S, e->stream, sel, odom, odom_stride);
      else drlgx_launch_sim(S, e->stream, sel, odom, odom_stride, n_measure);
    }
    {
      ScopedTimer t(e, 1);
      drlgx_launch_slam(S, e->stream, sel, pb);
    }
    {
      ScopedTimer t(e, 2);
      drlgx_launch_map(S, e->stream, sel, 1);
    }
  }
}

// the obstacle opt-in is live: asked for, and the ini file's [Environment] safe_distance can flag anything
static bool env_obstacles_on(const drlgx_engine *e) { return e->env_obstacles && e->S.cfg.safe_distance > 0.0; }

int drlgx_step(drlgx_engine *e, const double *odom_dev, const uint8_t *active_dev) {
  DRLGX_ENTER_OWING(e);
  if (!e || !odom_dev) return DRLGX_E_INVALID;
  LaunchSel sel{0, e->S.n_envs, active_dev, nullptr, 0};
  // every form of the step runs the map stage (kmap::map_body) and the SLAM stage's head (kslam::inc_settle or the fused step's own)
  // for every env: they take over what a lazy restore owes
  if (e->owed_slot >= 0) sel.vm_from = snapshot_base(e, e->owed_slot);
  e->owed_slot = -1;
  const int pb = std::min(max_bound(e) + 1, e->S.P_max);
  advance_pbound(e, 1);
  launch_belief_step(e, sel, odom_dev, 3, 2, pb, true, env_obstacles_on(e));
  {
    ScopedTimer t(e, 7);  // empty span: the event-pair overhead, so that callers can subtract it
  }
  return check_launch(e);
}

// One action index of the chosen plans of all envs (ExplorationEnv.step: `for a in actions: self._sim.simulate(a)`,
// scripts/envs/exploration_env.py:98-105): env i executes actions[i][action_index] while action_index < n_actions[i].
// map_last_only: the virtual map (a pure function of the SLAM state, rebuilt from the untouched map every time) is rebuilt
// at each env's LAST action only, and the marginals only where the map needs them - the state after the plan is the same.
int drlgx_step_plan(drlgx_engine *e, const double *actions_dev, const int32_t *n_actions_dev, int action_index, int map_last_only) {
  DRLGX_ENTER(e);
  if (!e || !actions_dev || !n_actions_dev || action_index < 0 || action_index >= e->S.A_max) return DRLGX_E_INVALID;
  LaunchSel sel{0, e->S.n_envs, nullptr, n_actions_dev, action_index};
  sel.map_last_only = map_last_only ? 1 : 0;
  const int pb = std::min(max_bound(e) + 1, e->S.P_max);
  advance_pbound(e, 1);
  launch_belief_step(e, sel, actions_dev, e->S.A_max * 3, 2, pb, false, env_obstacles_on(e));
  return check_launch(e);
}

// The look-ahead's simulator log: the simulator of every selected rollout over its whole action list first (k_presim, one wave per
// rollout; timer 0), replayed action by action by the steps that sel then launches.  No room for the log: the rollouts simulate
// inside their steps, from now on.
static void presimulate(drlgx_engine *e, LaunchSel &sel, const double *act, int n_measure, int max_n_actions) {
  const DrlgxState &S = e->S;
  const size_t entry = drlgx_simlog_entry_bytes(S), roll = entry * (size_t)S.A_max;
  if (!e->simlog_dev && dev_alloc(e, &e->simlog_dev, roll * (size_t)S.n_roll) != DRLGX_OK) {
    (void)hipGetLastError();
    e->last_error.clear();
    e->la_presim = false;
    return;
  }
  ScopedTimer t(e, 0);
  drlgx_launch_presim(S, e->stream, sel, act, S.A_max * 3, n_measure, max_n_actions, e->simlog_dev, roll, (int)entry);
  sel.simlog = e->simlog_dev;
  sel.simlog_roll = roll;
  sel.simlog_act = (int)entry;
}

// The actions [0, max_n_actions) of a selection's action lists (act: [sel.n][A_max][3]) as whole ranges per launch (k_step_loop /
// k_step_arrow_loop: a workgroup runs its instance's list); pbe: the pose bound before the first action.  Returns the first action
// index that is still to be launched one by one (launch_belief_step) - 0 when nothing was launched here.
// A launch per action index picks its kernel from the pose bound of THAT action (the fused dense-solver step while it serves the
// bound, then the step around the pose-chain solver); the loop form keeps that choice action by action - the leading actions
// [0, a_sw) in the dense loop kernel, the rest in the pose-chain one - because the two solvers round differently and the reference's
// integer worlds hold cells at exactly max_range from a pose: one ulp of a pose decides them, and with them O(0.1) of a reward.
// partial: when the pose-chain loop cannot take the rest, still run the dense loop for [0, a_sw) (else: nothing).
// presim: pre-simulate the lists (only when EVERY action is replayed: k_presim leaves the ground truth and the streams of the LAST action).
static int launch_action_range(drlgx_engine *e, LaunchSel sel, const double *act, int n_measure, int pbe, int max_n_actions, bool partial,
                               bool presim) {
  const DrlgxState &S = e->S;
  int a_sw = 0;
  while (a_sw < max_n_actions && drlgx_step_fusable(S, std::min(pbe + a_sw + 1, S.P_max))) ++a_sw;
  const bool rest_loops = a_sw == max_n_actions || drlgx_step_arrow_fusable(S);
  if (!e->la_loop || e->per_stage || !(rest_loops || (partial && a_sw > 0))) return 0;
  if (presim && e->la_presim && rest_loops) presimulate(e, sel, act, n_measure, max_n_actions);
  ScopedTimer t(e, 5);
  if (a_sw > 0) {
    sel.act_idx = 0;
    sel.pcap = std::min(pbe + 1, S.P_max);
    drlgx_launch_step_loop(S, e->stream, sel, act, S.A_max * 3, n_measure, a_sw);
  }
  if (a_sw == max_n_actions || !rest_loops) return a_sw;
  sel.act_idx = a_sw;
  sel.pcap = std::min(pbe + a_sw + 1, S.P_max);
  drlgx_launch_step_arrow_loop(S, e->stream, sel, act, S.A_max * 3, n_measure, max_n_actions);
  return max_n_actions;
}

// The whole loop `for a in actions: self._sim.simulate(a)` of every env (scripts/envs/exploration_env.py:98-105) in one call: env i
// executes actions[i][0 .. n_actions[i]); max_n_actions = a host-side bound of the plan lengths.  One launch when the fused
// step kernel serves every pose count the plans can reach (k_step_loop / k_step_arrow_loop: a workgroup runs its env's whole
// plan), else one drlgx_step_plan per action index.  Same results as that loop, bit for bit.
int drlgx_step_plans(drlgx_engine *e, const double *actions_dev, const int32_t *n_actions_dev, int max_n_actions, int map_last_only) {
  DRLGX_ENTER(e);
  if (!e || !actions_dev || !n_actions_dev || max_n_actions < 0 || max_n_actions > e->S.A_max) return DRLGX_E_INVALID;
  if (max_n_actions == 0) return DRLGX_OK;
  LaunchSel sel{0, e->S.n_envs, nullptr, n_actions_dev, 0};
  sel.map_last_only = map_last_only ? 1 : 0;
  // (all of them or none; under the obstacle opt-in none: every action raises or clears its env's flag in drlgx_step_plan's form)
  const int a_begin = env_obstacles_on(e) ? 0 : launch_action_range(e, sel, actions_dev, 2, max_bound(e), max_n_actions, false, false);
  advance_pbound(e, a_begin);
  for (int a = a_begin; a < max_n_actions; ++a) {
    const int r = drlgx_step_plan(e, actions_dev, n_actions_dev, a, map_last_only);
    if (r) return r;
  }
  return check_launch(e);
}

// The evaluation script's form of that loop (scripts/test.py:128-152): one launch per action index - the form whose intermediate
// maps are defined - with k_plan_record behind each: the metrics of every executed action, and an env that is done leaves its plan
// there (the record cuts n_actions_dev, which the later indices' launches read).  The host's pose bounds advance per launched index:
// an upper bound also for the envs that stop early.
int drlgx_step_plans_traced(drlgx_engine *e, const double *actions_dev, int32_t *n_actions_dev, int max_n_actions, double sigma0,
                            double done_explored, int max_steps, double *trace_dev, int32_t *done_dev) {
  DRLGX_ENTER(e);
  if (!e || !actions_dev || !n_actions_dev || !trace_dev || !done_dev || max_n_actions < 0 || max_n_actions > e->S.A_max)
    return DRLGX_E_INVALID;
  for (int a = 0; a < max_n_actions; ++a) {
    const int r = drlgx_step_plan(e, actions_dev, n_actions_dev, a, 0);
    if (r) return r;
    drlgx_launch_plan_record(e->S, e->stream, sigma0, a, n_actions_dev, done_explored, max_steps, trace_dev, done_dev);
  }
  return check_launch(e);
}

// A plan FOLLOWED (EMExplorer.follow_path, explore()'s switch on the planner's result: scripts/envs/pyplanner2d.py:100-109,170-187):
// k_follow_select turns (plan, result, steps) into every env's actions, then drlgx_step_plans_traced's loop with k_follow_record
// behind each action index, which also cuts at an obstacle flag and in front of a rejected odometry.  No host round trip.
int drlgx_follow_plans(drlgx_engine *e, const double *plan_dev, const int32_t *n_actions_dev, const int32_t *result_dev, const uint8_t *active_dev,
                       int steps, const double *fallback_xytheta, double sigma0, double done_explored, int max_steps, double *trace_dev,
                       int32_t *n_exec_dev, int32_t *done_dev, int32_t *stop_dev) {
  DRLGX_ENTER(e);
  if (!e || !plan_dev || !n_actions_dev || !result_dev || !fallback_xytheta || !trace_dev || !n_exec_dev || !done_dev || !stop_dev || steps < 0)
    return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  if (!e->follow_act) {
    int r = dev_alloc(e, &e->follow_act, (size_t)S.n_envs * S.A_max * 3);
    if (r) return r;
  }
  drlgx_launch_follow_select(S, e->stream, plan_dev, n_actions_dev, result_dev, active_dev, steps, fallback_xytheta, e->follow_act, n_exec_dev,
                             stop_dev);
  const int n_launch = std::min(std::max(steps, 1), S.A_max);  // (steps = 0 still runs a SAMPLING_FAILURE's fallback move)
  for (int a = 0; a < n_launch; ++a) {
    const int r = drlgx_step_plan(e, e->follow_act, n_exec_dev, a, 0);
    if (r) return r;
    drlgx_launch_follow_record(S, e->stream, sigma0, a, e->follow_act, n_exec_dev, env_obstacles_on(e) ? 1 : 0, done_explored, max_steps,
                               trace_dev, done_dev, stop_dev);
  }
  return check_launch(e);
}

int drlgx_set_env_obstacles(drlgx_engine *e, int enabled) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  // k_sim_step_obs keeps BOTH measure() calls' variates in LDS: an engine with more listed landmarks than that launch serves keeps
  // the opt-in off (its plain steps are not concerned)
  if (enabled && drlgx_sim_launch_lds(DRLGX_SIM_STEP_OBS, e->S.LG) > kSimLdsLimit) {
    e->env_obstacles = 0;
    e->last_error = "num_landmarks too large for the LDS of k_sim_step_obs: the obstacle opt-in stays off";
    return DRLGX_E_CAPACITY;
  }
  e->env_obstacles = enabled ? 1 : 0;
  return DRLGX_OK;
}

int drlgx_obstacle_flags(drlgx_engine *e, uint8_t *out_dev) {
  DRLGX_ENTER(e);
  if (!e || !out_dev) return DRLGX_E_INVALID;
  drlgx_launch_obstacle_flags(e->S, e->stream, out_dev);
  return check_launch(e);
}

// ---- staged form of the belief step: one call per call of SS2D.__init__ / SS2D.simulate (scripts/envs/pyss2d.py) -------
int drlgx_stage_reset_host(drlgx_engine *e, int n, const int32_t *env_ids, const uint32_t *seeds, const double *start) {
  DRLGX_ENTER(e);
  if (!e || n <= 0 || n > e->S.n_envs || !env_ids || !seeds || !start) return DRLGX_E_INVALID;
  for (int i = 0; i < n; ++i)
    if (env_ids[i] < 0 || env_ids[i] >= e->S.n_envs) return DRLGX_E_INVALID;
  HIPCHK(e, hipMemcpyAsync(e->stage_i32, env_ids, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->stage_u32, seeds, n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->stage_f64, start, n * 3 * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemsetAsync(e->S.status, 0, sizeof(int), e->stream));
  drlgx_launch_reset(e->S, e->stream, n, e->stage_i32, e->stage_u32, e->stage_f64, 0);
  for (int i = 0; i < n; ++i) e->pbound[env_ids[i]] = 1;
  int r = check_launch(e);
  if (r) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return DRLGX_OK;
}
int drlgx_stage_move(drlgx_engine *e, const double *odom_dev, const uint8_t *active_dev) {
  DRLGX_ENTER(e);
  if (!e || !odom_dev) return DRLGX_E_INVALID;
  advance_pbound(e, 1);
  drlgx_launch_sim_stage(e->S, e->stream, LaunchSel{0, e->S.n_envs, active_dev, nullptr, 0}, odom_dev, 0, nullptr, nullptr, nullptr);
  return check_launch(e);
}
int drlgx_stage_measure(drlgx_engine *e, const uint8_t *active_dev, int32_t *keys_dev, double *bearing_range_dev, int32_t *count_dev) {
  DRLGX_ENTER(e);
  if (!e || !keys_dev || !bearing_range_dev || !count_dev) return DRLGX_E_INVALID;
  HIPCHK(e, hipMemsetAsync(count_dev, 0, sizeof(int32_t) * e->S.n_envs, e->stream));
  drlgx_launch_sim_stage(e->S, e->stream, LaunchSel{0, e->S.n_envs, active_dev, nullptr, 0}, nullptr, 1, keys_dev, bearing_range_dev,
                         count_dev);
  return check_launch(e);
}
int drlgx_stage_add_measurements(drlgx_engine *e, const uint8_t *active_dev, const int32_t *keys_dev, const double *bearing_range_dev,
                                 const int32_t *count_dev) {
  DRLGX_ENTER(e);
  if (!e || !keys_dev || !bearing_range_dev || !count_dev) return DRLGX_E_INVALID;
  drlgx_launch_add_measurements(e->S, e->stream, LaunchSel{0, e->S.n_envs, active_dev, nullptr, 0}, keys_dev, bearing_range_dev, count_dev);
  return check_launch(e);
}
int drlgx_stage_optimize(drlgx_engine *e, const uint8_t *active_dev) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  drlgx_launch_slam(e->S, e->stream, LaunchSel{0, e->S.n_envs, active_dev, nullptr, 0}, max_bound(e));
  return check_launch(e);
}
int drlgx_stage_update_map(drlgx_engine *e, const uint8_t *active_dev, int rebuild) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  drlgx_launch_map(e->S, e->stream, LaunchSel{0, e->S.n_envs, active_dev, nullptr, 0}, rebuild ? 1 : 0);
  return check_launch(e);
}

// a scratch array of at least `count` elements: kept while it is large enough, replaced (behind the stream's work) when it is not
extern "C++" {
template <typename T>
static int scratch_reserve(drlgx_engine *e, T **p, size_t count) {
  if (*p) {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), (void *)*p), e->allocs.end());
    HIPCHK(e, hipFree(*p));
    *p = nullptr;
  }
  return dev_alloc(e, p, count);
}
}

// FastMarginals2::update for candidate action lists (k_fm2.hip)
static const int kFm2Chunk = 128;
using kfm2::kFm2MaxMeas;
// What the entries below do with their candidates: the workspaces on first use, the prior covariance of every environment, then
// one update launch per kFm2Chunk candidates.  cov_out / n_out hold all n_cand candidates - or, chunk_out, only the chunk at hand,
// which after(c0, nc) consumes on the engine's stream before the next chunk's launch overwrites it.  lm_out (null: the kernels as
// they were without it): the landmark blocks as well, [.][L_max][3], all candidates or (lm_chunk) the chunk at hand; the prior is
// then summed in a fixed order (k_fm2_prior_ordered), so that such a call gives the same bits whenever it is repeated.
static int fm2_run(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                   const uint8_t *core_dev, double *cov_out, int out_stride_poses, int32_t *n_out, bool chunk_out, const std::function<void(int, int)> &after,
                   double *lm_out = nullptr, bool lm_chunk = false) {
  const DrlgxState &S = e->S;
  if (!e->fm2_sig) {
    const size_t nmax = (size_t)3 * S.P_max + 2 * S.L_max;
    e->fm2_sig_stride = nmax * nmax;
    int r;
    if ((r = dev_alloc(e, &e->fm2_sig, e->fm2_sig_stride * (size_t)S.n_envs))) return r;
    if ((r = dev_alloc(e, &e->fm2_scratch, drlgx_fm2_scratch_doubles(S) * (size_t)kFm2Chunk))) return r;
    if ((r = dev_alloc(e, &e->fm2_iscratch, kfm2::Fm2Scratch(S.A_max, kFm2MaxMeas).itotal * (size_t)kFm2Chunk))) return r;
  }
  if (lm_out)
    drlgx_launch_fm2_prior_ordered(S, e->stream, e->fm2_sig, e->fm2_sig_stride, 3 * S.P_max + 2 * S.L_max);
  else
    drlgx_launch_fm2_prior(S, e->stream, e->fm2_sig, e->fm2_sig_stride, 3 * S.P_max + 2 * S.L_max);
  for (int c0 = 0; c0 < n_cand; c0 += kFm2Chunk) {
    const int nc = std::min(kFm2Chunk, n_cand - c0);
    drlgx_launch_fm2_update(S, e->stream, nc, cand_env_dev + c0, actions_dev + (size_t)c0 * S.A_max * 3, n_actions_dev + c0,
                            core_dev ? core_dev + (size_t)c0 * S.A_max : nullptr, e->fm2_sig, e->fm2_sig_stride, e->fm2_scratch, e->fm2_iscratch,
                            chunk_out ? cov_out : cov_out + (size_t)c0 * out_stride_poses * 9, out_stride_poses,
                            chunk_out ? n_out : n_out + c0, (!lm_out || lm_chunk) ? lm_out : lm_out + (size_t)c0 * S.L_max * 3, S.L_max);
    after(c0, nc);
  }
  return check_launch(e);
}

// core_dev (null: every action is a core pose): a non-core step gets its pose and its odometry factor and predicts no measurement
int drlgx_fm2_update_steps(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                           const uint8_t *core_dev, double *cov_out_dev, int out_stride_poses, int32_t *n_out_dev) {
  DRLGX_ENTER(e);
  if (!e || n_cand < 0 || !cand_env_dev || !actions_dev || !n_actions_dev || !cov_out_dev || !n_out_dev ||
      out_stride_poses < e->S.P_max + e->S.A_max)
    return DRLGX_E_INVALID;
  if (n_cand == 0) return DRLGX_OK;
  return fm2_run(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev, cov_out_dev, out_stride_poses, n_out_dev, false,
                 [](int, int) {});
}
int drlgx_fm2_update(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                     double *cov_out_dev, int out_stride_poses, int32_t *n_out_dev) {
  return drlgx_fm2_update_steps(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, nullptr, cov_out_dev, out_stride_poses, n_out_dev);
}

// One check launch and its answer: the flag word zeroed, launch(flag) on the engine's stream, the flag read back - the smallest
// DRLGX_E_* code a candidate earns, 0 if none does.  The read is a call's single synchronisation.
static int run_check(drlgx_engine *e, const std::function<void(int *)> &launch) {
  if (!e->check_flag) {
    if (int r = dev_alloc(e, &e->check_flag, (size_t)1)) return r;
  }
  int flag = 0;
  HIPCHK(e, hipMemsetAsync(e->check_flag, 0, sizeof(int), e->stream));
  launch(e->check_flag);
  HIPCHK(e, hipMemcpyAsync(&flag, e->check_flag, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return flag;
}

// The leaf evaluation of EMPlanner2D::optimize2 for candidate action lists: the covariance update above into the engine's scratch,
// a chunk at a time, and k_em.hip on each chunk.  What the kernels could only report through the status word - a candidate that
// names no environment, a plan beyond max_actions, more than kFm2MaxMeas predicted measurements - is found out first (run_check),
// so that such a call returns its code and leaves the status word alone.  core_dev / distance_dev (either may be null): the leaves
// of a tree whose edges have non-core steps - only core poses predict measurements and enter the leaf's map, the cost takes the
// tree's distance.
// The chunk workspaces of em_cost_run (on first use) and its check of the candidates.
static int em_cost_check(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                         const uint8_t *core_dev) {
  const DrlgxState &S = e->S;
  if (!e->em_cov) {
    int r;
    if ((r = dev_alloc(e, &e->em_cov, (size_t)kFm2Chunk * (S.P_max + S.A_max) * 9))) return r;
    if ((r = dev_alloc(e, &e->em_nout, (size_t)kFm2Chunk))) return r;
  }
  return run_check(e, [&](int *flag) { drlgx_launch_fm2_check(S, e->stream, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev, flag); });
}

static int em_cost_run(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                       const uint8_t *core_dev, const double *distance_dev, int algorithm, double *uncertainty_out_dev, double *cost_out_dev, double *info_out_dev) {
  const DrlgxState &S = e->S;
  if (drlgx_em_lds_bytes(S) > (size_t)160 * 1024) return DRLGX_E_CAPACITY;
  const int stride = S.P_max + S.A_max;
  if (int flag = em_cost_check(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev)) return flag;
  return fm2_run(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev, e->em_cov, stride, e->em_nout, true, [&](int c0, int nc) {
    drlgx_launch_em_cost(S, e->stream, nc, cand_env_dev + c0, actions_dev + (size_t)c0 * S.A_max * 3, n_actions_dev + c0,
                         core_dev ? core_dev + (size_t)c0 * S.A_max : nullptr, distance_dev ? distance_dev + c0 : nullptr, e->em_cov, stride,
                         algorithm, uncertainty_out_dev ? uncertainty_out_dev + c0 : nullptr, cost_out_dev ? cost_out_dev + c0 : nullptr,
                         info_out_dev ? info_out_dev + (size_t)c0 * S.V * 3 : nullptr);
  });
}

int drlgx_em_cost_steps(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                        const uint8_t *core_dev, const double *distance_dev, int algorithm, double *uncertainty_out_dev,
                        double *cost_out_dev, double *info_out_dev) {
  DRLGX_ENTER(e);
  if (!e || n_cand < 0 || !cand_env_dev || !actions_dev || !n_actions_dev || (!uncertainty_out_dev && !cost_out_dev) ||
      (algorithm != DRLGX_ALG_EM_AOPT && algorithm != DRLGX_ALG_EM_DOPT))
    return DRLGX_E_INVALID;
  if (n_cand == 0) return DRLGX_OK;
  return em_cost_run(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev, distance_dev, algorithm, uncertainty_out_dev,
                     cost_out_dev, info_out_dev);
}
int drlgx_em_cost(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                  int algorithm, double *uncertainty_out_dev, double *cost_out_dev, double *info_out_dev) {
  return drlgx_em_cost_steps(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, nullptr, nullptr, algorithm, uncertainty_out_dev,
                             cost_out_dev, info_out_dev);
}

// calculateUncertainty_OG_SHANNON + costFunction for candidate action lists (k_og.hip).  The candidates are checked first, as in
// em_cost_run: one small launch and one read of its flag, so that a refused call leaves the status word alone.  No covariance, no
// scratch per candidate: all candidates go in one launch.
int drlgx_og_cost(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                  double *entropy_out_dev, double *cost_out_dev, double *prob_out_dev) {
  DRLGX_ENTER(e);
  if (!e || n_cand < 0) return DRLGX_E_INVALID;
  if (n_cand == 0) return DRLGX_OK;  // (no array is read: empty ones may be null)
  if (!cand_env_dev || !actions_dev || !n_actions_dev || (!entropy_out_dev && !cost_out_dev)) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  if (drlgx_og_lds_bytes(S) > (size_t)160 * 1024) return DRLGX_E_CAPACITY;
  if (int flag = run_check(e, [&](int *f) { drlgx_launch_og_check(S, e->stream, n_cand, cand_env_dev, n_actions_dev, f); })) return flag;
  drlgx_launch_og_cost(S, e->stream, n_cand, cand_env_dev, actions_dev, n_actions_dev, entropy_out_dev, cost_out_dev, prob_out_dev);
  return check_launch(e);
}

// calculateUncertainty_SLAM_OG_SHANNON + costFunction for candidate action lists: the root's weights from the live belief, the leaf
// entropy of every candidate (k_og.hip, one launch, as drlgx_og_cost), then the fm2 update with its landmark blocks a chunk at a time
// and the blend on each chunk.  The candidates are checked first exactly as em_cost_run checks them - the call's one synchronisation.
// The entropy, cost and distance factors (any of them null) of candidates that are the leaves of sampling trees over env_sel [n_sel]:
// the part the leaves of a tree share once per environment, then the leaves (k_og_tree_base + k_og_tree_cost) - or, under
// DRLGX_OG_TREE_SHARED=0, k_og_cost on every leaf.  The same bits either way.
static int og_tree_leaves(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, int n_cand, const int32_t *cand_env_dev,
                          const double *actions_dev, const int32_t *n_actions_dev, double *ent_out, double *cost_out, double *dist_out) {
  const DrlgxState &S = e->S;
  if (e->og_tree_shared && !e->og_base) {
    int r;
    if ((r = dev_alloc(e, &e->og_base, (size_t)S.n_envs * S.Vu))) return r;
    if ((r = dev_alloc(e, &e->og_known, (size_t)S.n_envs))) return r;
  }
  ScopedTimer t(e, 6);  // (the A/B of profiles/og_plan_shared_vs_unshared.txt)
  if (!e->og_tree_shared) {
    drlgx_launch_og_cost(S, e->stream, n_cand, cand_env_dev, actions_dev, n_actions_dev, ent_out, cost_out, nullptr, dist_out);
    return DRLGX_OK;
  }
  drlgx_launch_og_tree_cost(S, e->stream, n_sel, env_sel_dev, n_cand, cand_env_dev, actions_dev, n_actions_dev, e->og_base, e->og_known,
                            ent_out, cost_out, dist_out);
  return DRLGX_OK;
}

// The body of drlgx_slam_og_cost.  tree_sel_dev [n_tree_sel] (or null): the candidates are the leaves of trees over these
// environments (drlgx_og_plan) - their entropy comes from og_tree_leaves.
static int slam_og_run(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                       const uint8_t *core_dev, const double *distance_dev, double alpha, double *uncertainty_out_dev, double *cost_out_dev,
                       double *terms_out_dev, double *weights_out_dev, double *lm_cov_out_dev, int n_tree_sel, const int32_t *tree_sel_dev) {
  const DrlgxState &S = e->S;
  if (drlgx_og_lds_bytes(S) > (size_t)160 * 1024) return DRLGX_E_CAPACITY;
  int r;
  if (!e->sog_weights) {
    if ((r = dev_alloc(e, &e->sog_weights, (size_t)2 * S.n_envs))) return r;
    if ((r = dev_alloc(e, &e->sog_lm, (size_t)kFm2Chunk * S.L_max * 3))) return r;
  }
  if ((size_t)n_cand > e->sog_cap) {
    if ((r = scratch_reserve(e, &e->sog_h, (size_t)n_cand))) return r;
    if ((r = scratch_reserve(e, &e->sog_dist, (size_t)2 * n_cand))) return r;
    e->sog_cap = (size_t)n_cand;
  }
  if (int flag = em_cost_check(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev)) return flag;
  double *weights = weights_out_dev ? weights_out_dev : e->sog_weights;
  drlgx_launch_slam_og_weights(S, e->stream, alpha, weights);
  if (!tree_sel_dev)
    drlgx_launch_og_cost(S, e->stream, n_cand, cand_env_dev, actions_dev, n_actions_dev, e->sog_h, nullptr, nullptr, e->sog_dist);
  else if ((r = og_tree_leaves(e, n_tree_sel, tree_sel_dev, n_cand, cand_env_dev, actions_dev, n_actions_dev, e->sog_h, nullptr, e->sog_dist)))
    return r;
  return fm2_run(
      e, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev, e->em_cov, S.P_max + S.A_max, e->em_nout, true,
      [&](int c0, int nc) {
        drlgx_launch_slam_og_blend(S, e->stream, nc, cand_env_dev + c0, lm_cov_out_dev ? lm_cov_out_dev + (size_t)c0 * S.L_max * 3 : e->sog_lm,
                                   S.L_max, e->sog_h + c0, e->sog_dist + (size_t)2 * c0, distance_dev ? distance_dev + c0 : nullptr, weights,
                                   uncertainty_out_dev ? uncertainty_out_dev + c0 : nullptr, cost_out_dev + c0,
                                   terms_out_dev ? terms_out_dev + (size_t)2 * c0 : nullptr);
      },
      lm_cov_out_dev ? lm_cov_out_dev : e->sog_lm, lm_cov_out_dev == nullptr);
}

int drlgx_slam_og_cost(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev, const int32_t *n_actions_dev,
                       const uint8_t *core_dev, const double *distance_dev, double alpha, double *uncertainty_out_dev, double *cost_out_dev,
                       double *terms_out_dev, double *weights_out_dev, double *lm_cov_out_dev) {
  DRLGX_ENTER(e);
  if (!e || n_cand <= 0 || !cand_env_dev || !actions_dev || !n_actions_dev || !uncertainty_out_dev || !cost_out_dev ||
      !(alpha >= 0.0 && alpha <= 1.0))
    return DRLGX_E_INVALID;
  return slam_og_run(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, core_dev, distance_dev, alpha, uncertainty_out_dev, cost_out_dev,
                     terms_out_dev, weights_out_dev, lm_cov_out_dev, 0, nullptr);
}

// ---- the EM planner's tree sampler (k_em_tree.hip) ----
static const int kTreeMaxNodes = 2048, kTreeMeta = 4;

int drlgx_set_sampler_parameter(drlgx_engine *e, double max_nodes, double safe_distance, int dubins_control_model_enabled) {
  DRLGX_ENTER(e);
  if (!e || !(max_nodes >= 0.0)) return DRLGX_E_INVALID;
  e->sampler_max_nodes = max_nodes;
  e->sampler_safe_distance = safe_distance;
  e->sampler_dubins = dubins_control_model_enabled ? 1 : 0;
  return DRLGX_OK;
}

int drlgx_set_sampler_obstacles(drlgx_engine *e, int enabled) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  e->sampler_obstacles = enabled ? 1 : 0;
  return DRLGX_OK;
}

int drlgx_set_dubins_leaf_scoring(drlgx_engine *e, int enabled) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  e->dubins_leaf_scoring = enabled ? 1 : 0;
  return DRLGX_OK;
}

// ---- the Dubins path library (EMPlanner2D::initializeDubinsPathLibrary, Planner2D.cpp:1359-1414) ----
static const int kDubinsMaxEntries = 131072;  // (the [Dubins] section scripts/envs/pyplanner2d.ini ships gives 78 030)
static const int kDubinsMaxSteps = 4096;      // steps of one path
static const int kDubinsMaxPairs = 1 << 20;   // (v, w) pairs looked at, entries or not

int drlgx_set_dubins_library_host(drlgx_engine *e, const double *params) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  if (!params) {
    e->dubins = DrlgxDubins{};
    e->dub_end_h.clear(); e->dub_v_h.clear(); e->dub_w_h.clear(); e->dub_steps_h.clear();
    return DRLGX_OK;
  }
  const double max_w = params[0], dw = params[1], min_v = params[2], max_v = params[3], dv = params[4], dt = params[5];
  const double min_duration = params[6], max_duration = params[7], tol = params[8];
  if (!(max_w > 0.0) || !(dw > 0.0) || !(dv > 0.0) || !(dt > 0.0) || !(tol > 0.0) || !(max_v >= min_v) || !std::isfinite(max_w) ||
      !std::isfinite(max_v) || !std::isfinite(min_v) || !std::isfinite(tol) || !std::isfinite(min_duration) || !std::isfinite(max_duration))
    return DRLGX_E_INVALID;
  // the loops as the reference writes them: the counts come from this floating-point arithmetic, not from a division
  std::vector<double> end, vv, ww, ex, ey;
  std::vector<int> steps;
  int pairs = 0, max_steps = 0;
  double reach = 0.0;
  for (double v = max_v; v > min_v - 1e-10; v -= dv) {
    for (double w = 0; w < max_w + 1e-10; w += dw) {
      if (++pairs > kDubinsMaxPairs) return DRLGX_E_CAPACITY;
      for (int s = -1; s <= 1; s += 2) {
        double t = 0.0;
        const double wws = w * s;
        double x = 0.0, y = 0.0, c = 1.0, sn = 0.0;  // Pose2(0, 0, 0)
        int num_steps = 0;
        while (t < max_duration) {
          if (++num_steps > kDubinsMaxSteps) return DRLGX_E_CAPACITY;
          const double nx = x + v * dt * c, ny = y + v * dt * sn, th = std::atan2(sn, c) + wws * dt;
          x = nx; y = ny; c = std::cos(th); sn = std::sin(th);  // Pose2(x, y, theta)
          t += dt;
          if (t > min_duration) {
            if (steps.size() >= (size_t)kDubinsMaxEntries) return DRLGX_E_CAPACITY;
            end.push_back(x); end.push_back(y); end.push_back(std::atan2(sn, c));
            ex.push_back(x); ey.push_back(y);
            vv.push_back(v); ww.push_back(wws); steps.push_back(num_steps);
            max_steps = std::max(max_steps, num_steps);
            reach = std::max(reach, std::sqrt(x * x + y * y));
          }
        }
      }
    }
  }
  if (steps.empty()) return DRLGX_E_INVALID;  // (no path lasts longer than min_duration: nothing could ever connect)
  const size_t n = steps.size();
  int r;
  if (n > e->dub_cap) {
    if ((r = scratch_reserve(e, &e->dub_end_x, n))) return r;
    if ((r = scratch_reserve(e, &e->dub_end_y, n))) return r;
    if ((r = scratch_reserve(e, &e->dub_v, n))) return r;
    if ((r = scratch_reserve(e, &e->dub_w, n))) return r;
    if ((r = scratch_reserve(e, &e->dub_steps, n))) return r;
    e->dub_cap = n;
  }
  HIPCHK(e, hipMemcpyAsync(e->dub_end_x, ex.data(), n * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->dub_end_y, ey.data(), n * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->dub_v, vv.data(), n * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->dub_w, ww.data(), n * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->dub_steps, steps.data(), n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // (the host buffers end with this call)
  // the exact pre-filter's bound: |local| beyond it implies |local - end_i| > tol for every i (triangle inequality); the factor
  // covers the roundings of the square roots and of this sum many times over
  e->dub_reach = (reach + tol) * (1.0 + 9.313225746154785e-10);
  e->dubins = DrlgxDubins{e->dub_end_x, e->dub_end_y, e->dub_v, e->dub_w, e->dub_steps, (int)n, max_steps, dt, tol,
                          e->dub_prefilter ? e->dub_reach : HUGE_VAL, nullptr};
  e->dub_end_h.swap(end); e->dub_v_h.swap(vv); e->dub_w_h.swap(ww); e->dub_steps_h.swap(steps);
  return DRLGX_OK;
}

int drlgx_set_dubins_prefilter(drlgx_engine *e, int enabled) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  e->dub_prefilter = enabled ? 1 : 0;
  if (e->dubins.n > 0) e->dubins.reach = e->dub_prefilter ? e->dub_reach : HUGE_VAL;
  return DRLGX_OK;
}

int drlgx_dubins_library(drlgx_engine *e, int capacity, int32_t *n_out, double *end_xytheta, double *v, double *w, int32_t *num_steps) {
  DRLGX_ENTER(e);
  if (!e || !n_out || capacity < 0) return DRLGX_E_INVALID;
  const int n = (int)e->dub_steps_h.size();
  *n_out = n;
  const int m = std::min(n, capacity);
  if (end_xytheta) std::copy(e->dub_end_h.begin(), e->dub_end_h.begin() + (size_t)3 * m, end_xytheta);
  if (v) std::copy(e->dub_v_h.begin(), e->dub_v_h.begin() + m, v);
  if (w) std::copy(e->dub_w_h.begin(), e->dub_w_h.begin() + m, w);
  if (num_steps) std::copy(e->dub_steps_h.begin(), e->dub_steps_h.begin() + m, num_steps);
  return DRLGX_OK;
}

// Grows the trees and reads their results back: meta_h[n_sel][kTreeMeta] and the flag - the one synchronisation.  Returns the
// flag's code when a tree was refused.
static int tree_grow(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *halton_start_dev, int cap, int mode,
                     const int32_t *goal_key_dev, const double *goal_xy_dev, double *nodes_out_dev, int32_t *n_nodes_out_dev,
                     int32_t *result_out_dev, int32_t *halton_next_out_dev, std::vector<int> &meta_h) {
  int r;
  const bool dubins = e->sampler_dubins != 0;  // (tree_args_ok: a library is loaded; mode 0 behind drlgx_set_dubins_leaf_scoring)
  if ((size_t)n_sel > e->tree_sel_cap) {
    if ((r = scratch_reserve(e, &e->tree_meta, (size_t)n_sel * kTreeMeta + 1))) return r;  // (+ the flag, behind the trees' rows)
    e->tree_sel_cap = (size_t)n_sel;
    e->tree_nodes_cap = 0;
  }
  const size_t nodes = (size_t)n_sel * cap;
  if (nodes > e->tree_nodes_cap) {
    if ((r = scratch_reserve(e, &e->tree_act, nodes * 3))) return r;
    if ((r = scratch_reserve(e, &e->tree_link, nodes * 2))) return r;
    if ((r = scratch_reserve(e, &e->tree_leaf, nodes))) return r;
    e->tree_nodes_cap = nodes;
  }
  if (dubins && nodes > e->tree_pose_cap) {
    if ((r = scratch_reserve(e, &e->tree_pose, nodes * 4))) return r;
    e->tree_pose_cap = nodes;
  }
  e->dubins.pose = e->tree_pose;
  int *flag_dev = e->tree_meta + (size_t)n_sel * kTreeMeta;
  HIPCHK(e, hipMemsetAsync(flag_dev, 0, sizeof(int), e->stream));
  // (the obstacle logic only where there is a distance to keep: at exactly 0 the plain growth loop is the same tree)
  const bool obstacles = e->sampler_obstacles && e->sampler_safe_distance != 0.0;
  const DrlgxTreeArgs args = {n_sel, env_sel_dev, halton_start_dev, cap, mode, e->sampler_max_nodes, e->sampler_safe_distance,
                              goal_key_dev, goal_xy_dev, e->tree_act, e->tree_link, e->tree_leaf, e->tree_meta, flag_dev,
                              nodes_out_dev, n_nodes_out_dev, result_out_dev, halton_next_out_dev, e->dubins};
  drlgx_launch_em_tree(e->S, e->stream, args, obstacles, dubins);
  if ((r = check_launch(e))) return r;
  meta_h.resize((size_t)n_sel * kTreeMeta + 1);
  HIPCHK(e, hipMemcpyAsync(meta_h.data(), e->tree_meta, meta_h.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return meta_h.back();
}

// The Dubins control model is served where a library is loaded (drlgx_set_dubins_library_host, the opt-in) and the planner is
// rrt_planner - or optimize2 behind its own opt-in, drlgx_set_dubins_leaf_scoring; everywhere else the flag is refused.
static bool tree_args_ok(const drlgx_engine *e, int n_sel, const void *env_sel, const void *halton_start, int cap, const void *plan_out,
                         const void *n_actions_out, bool rrt) {
  return e && n_sel >= 0 && env_sel && halton_start && plan_out && n_actions_out && cap >= 1 && cap <= kTreeMaxNodes &&
         (e->sampler_obstacles ? e->sampler_safe_distance >= 0.0 : e->sampler_safe_distance == 0.0) &&
         (!e->sampler_dubins || (e->dubins.n > 0 && (rrt || e->dubins_leaf_scoring)));
}

// What the outputs of a tree call point to (drlgx_em_plan's argument list)
struct TreePlanOut {
  double *plan, *cost, *nodes;
  int32_t *n_actions, *result, *n_leaves, *halton_next, *n_nodes;
};

// optimize2 behind the entries' own argument checks: the trees (tree_grow: the call's first synchronisation), their leaves as
// candidates in the engine's tables (k_em_leaves, or its Dubins form under the sampler's flag), score(n_cand, steps) - which leaves
// every candidate's cost in e->tree_cost - and the pick.  What the entries differ in is `score` alone.
static int tree_plan(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *halton_start_dev, int max_tree_nodes,
                     const TreePlanOut &o, const std::function<int(int, bool)> &score) {
  const DrlgxState &S = e->S;
  std::vector<int> meta;
  int r = tree_grow(e, n_sel, env_sel_dev, halton_start_dev, max_tree_nodes, 0, nullptr, nullptr, o.nodes, o.n_nodes, o.result,
                    o.halton_next, meta);
  if (r) return r;
  size_t n_cand = 0;
  for (int i = 0; i < n_sel; ++i) n_cand += (size_t)meta[(size_t)i * kTreeMeta + 1];
  if (n_cand > (size_t)0x7fffffff) return DRLGX_E_CAPACITY;
  if (n_cand > e->tree_cand_cap) {
    if ((r = scratch_reserve(e, &e->tree_cand_act, n_cand * S.A_max * 3))) return r;
    if ((r = scratch_reserve(e, &e->tree_cand_env, n_cand))) return r;
    if ((r = scratch_reserve(e, &e->tree_cand_n, n_cand))) return r;
    if ((r = scratch_reserve(e, &e->tree_cost, n_cand))) return r;
    e->tree_cand_cap = n_cand;
  }
  const bool steps = e->sampler_dubins != 0;  // the leaves have non-core steps: one row per step, the mask, the tree's distance
  if (steps && n_cand > e->tree_cand_steps_cap) {
    if ((r = scratch_reserve(e, &e->tree_cand_core, n_cand * S.A_max))) return r;
    if ((r = scratch_reserve(e, &e->tree_cand_dist, n_cand))) return r;
    e->tree_cand_steps_cap = n_cand;
  }
  e->tree_cand_last = 0;
  if (n_cand > 0) {  // (every tree failed to sample: nothing to score, the pick below writes the empty plans)
    if (steps)
      drlgx_launch_em_leaves_dubins(e->stream, n_sel, env_sel_dev, max_tree_nodes, S.A_max, S.cfg.angle_weight, e->tree_act, e->tree_link,
                                    e->tree_leaf, e->tree_meta, e->dubins, 0, e->tree_cand_env, e->tree_cand_act, e->tree_cand_n,
                                    e->tree_cand_core, e->tree_cand_dist);
    else
      drlgx_launch_em_leaves(e->stream, n_sel, env_sel_dev, max_tree_nodes, S.A_max, e->tree_act, e->tree_link, e->tree_leaf, e->tree_meta,
                             0, e->tree_cand_env, e->tree_cand_act, e->tree_cand_n);
    if ((r = check_launch(e))) return r;
    if ((r = score((int)n_cand, steps))) return r;
    e->tree_cand_last = n_cand;
    e->tree_cand_last_steps = steps;
  }
  drlgx_launch_em_pick(e->stream, n_sel, S.A_max, e->tree_meta, e->tree_cost, e->tree_cand_act, e->tree_cand_n, o.plan, o.n_actions, o.cost,
                       o.n_leaves);
  return check_launch(e);
}

int drlgx_em_plan(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *halton_start_dev, int max_tree_nodes,
                  int algorithm, double *plan_out_dev, int32_t *n_actions_out_dev, double *cost_out_dev, int32_t *result_out_dev,
                  int32_t *n_leaves_out_dev, int32_t *halton_next_out_dev, double *nodes_out_dev, int32_t *n_nodes_out_dev) {
  DRLGX_ENTER(e);
  if (!tree_args_ok(e, n_sel, env_sel_dev, halton_start_dev, max_tree_nodes, plan_out_dev, n_actions_out_dev, false) ||
      (algorithm != DRLGX_ALG_EM_AOPT && algorithm != DRLGX_ALG_EM_DOPT))
    return DRLGX_E_INVALID;
  if (n_sel == 0) return DRLGX_OK;
  const TreePlanOut out = {plan_out_dev, cost_out_dev, nodes_out_dev, n_actions_out_dev, result_out_dev, n_leaves_out_dev,
                           halton_next_out_dev, n_nodes_out_dev};
  return tree_plan(e, n_sel, env_sel_dev, halton_start_dev, max_tree_nodes, out, [&](int n_cand, bool steps) {
    return em_cost_run(e, n_cand, e->tree_cand_env, e->tree_cand_act, e->tree_cand_n, steps ? e->tree_cand_core : nullptr,
                       steps ? e->tree_cand_dist : nullptr, algorithm, nullptr, e->tree_cost, nullptr);
  });
}

// optimize2 under OG_SHANNON / SLAM_OG_SHANNON: drlgx_em_plan's tree, leaves and pick (tree_plan), the leaves scored by og_tree_leaves
// (algorithm 2: no check of the candidates - the tree's own flag has refused a leaf deeper than max_actions - and so no second
// synchronisation) or by the body of drlgx_slam_og_cost (algorithm 3: its candidate check is the second one).
int drlgx_og_plan(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *halton_start_dev, int max_tree_nodes,
                  int algorithm, double alpha, double *plan_out_dev, int32_t *n_actions_out_dev, double *cost_out_dev,
                  int32_t *result_out_dev, int32_t *n_leaves_out_dev, int32_t *halton_next_out_dev, double *nodes_out_dev,
                  int32_t *n_nodes_out_dev) {
  DRLGX_ENTER(e);
  if (!tree_args_ok(e, n_sel, env_sel_dev, halton_start_dev, max_tree_nodes, plan_out_dev, n_actions_out_dev, false) ||
      (algorithm != DRLGX_ALG_OG_SHANNON && algorithm != DRLGX_ALG_SLAM_OG_SHANNON) || e->sampler_dubins ||
      (algorithm == DRLGX_ALG_SLAM_OG_SHANNON && !(alpha >= 0.0 && alpha <= 1.0)))
    return DRLGX_E_INVALID;
  if (n_sel == 0) return DRLGX_OK;
  if (drlgx_og_lds_bytes(e->S) > (size_t)160 * 1024) return DRLGX_E_CAPACITY;
  const TreePlanOut out = {plan_out_dev, cost_out_dev, nodes_out_dev, n_actions_out_dev, result_out_dev, n_leaves_out_dev,
                           halton_next_out_dev, n_nodes_out_dev};
  return tree_plan(e, n_sel, env_sel_dev, halton_start_dev, max_tree_nodes, out, [&](int n_cand, bool) {
    if (algorithm == DRLGX_ALG_SLAM_OG_SHANNON)
      return slam_og_run(e, n_cand, e->tree_cand_env, e->tree_cand_act, e->tree_cand_n, nullptr, nullptr, alpha, nullptr, e->tree_cost,
                         nullptr, nullptr, nullptr, n_sel, env_sel_dev);
    if (int r = og_tree_leaves(e, n_sel, env_sel_dev, n_cand, e->tree_cand_env, e->tree_cand_act, e->tree_cand_n, nullptr, e->tree_cost, nullptr))
      return r;
    return check_launch(e);
  });
}

// The leaves the last served drlgx_em_plan or drlgx_og_plan scored, as it handed them to the body of drlgx_em_cost_steps (of
// drlgx_og_cost / drlgx_slam_og_cost), with the costs that call computed: device-to-device copies on the engine's stream.
int drlgx_em_plan_leaves(drlgx_engine *e, int capacity, int32_t *n_out_host, int32_t *has_steps_out_host, int32_t *cand_env_out_dev,
                         double *actions_out_dev, int32_t *n_actions_out_dev, uint8_t *core_out_dev, double *distance_out_dev,
                         double *cost_out_dev) {
  DRLGX_ENTER(e);
  if (!e || !n_out_host || capacity < 0) return DRLGX_E_INVALID;
  const size_t n = e->tree_cand_last, m = std::min(n, (size_t)capacity), A = (size_t)e->S.A_max;
  const bool steps = e->tree_cand_last_steps;
  if (m > 0 && !steps && distance_out_dev) return DRLGX_E_INVALID;  // (no distance was kept: refused before anything is written)
  *n_out_host = (int32_t)n;
  if (has_steps_out_host) *has_steps_out_host = steps ? 1 : 0;
  if (m == 0) return DRLGX_OK;
  auto copy = [&](void *dst, const void *src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, e->stream) : hipSuccess;
  };
  HIPCHK(e, copy(cand_env_out_dev, e->tree_cand_env, m * sizeof(int32_t)));
  HIPCHK(e, copy(actions_out_dev, e->tree_cand_act, m * A * 3 * sizeof(double)));
  HIPCHK(e, copy(n_actions_out_dev, e->tree_cand_n, m * sizeof(int32_t)));
  HIPCHK(e, copy(cost_out_dev, e->tree_cost, m * sizeof(double)));
  if (steps) {
    HIPCHK(e, copy(core_out_dev, e->tree_cand_core, m * A));
    HIPCHK(e, copy(distance_out_dev, e->tree_cand_dist, m * sizeof(double)));
  } else {  // every action a core pose; the distance is the plan's own: none is kept
    if (core_out_dev) HIPCHK(e, hipMemsetAsync(core_out_dev, 1, m * A, e->stream));
  }
  return DRLGX_OK;
}

int drlgx_rrt_plan(drlgx_engine *e, int n_sel, const int32_t *env_sel_dev, const int32_t *goal_key_dev, const double *goal_xy_dev,
                   const int32_t *halton_start_dev, int max_tree_nodes, double *plan_out_dev, int32_t *n_actions_out_dev,
                   int32_t *result_out_dev, int32_t *halton_next_out_dev, double *nodes_out_dev, int32_t *n_nodes_out_dev) {
  DRLGX_ENTER(e);
  if (!tree_args_ok(e, n_sel, env_sel_dev, halton_start_dev, max_tree_nodes, plan_out_dev, n_actions_out_dev, true) || !goal_key_dev ||
      !goal_xy_dev)
    return DRLGX_E_INVALID;
  if (n_sel == 0) return DRLGX_OK;
  std::vector<int> meta;
  int r = tree_grow(e, n_sel, env_sel_dev, halton_start_dev, max_tree_nodes, 1, goal_key_dev, goal_xy_dev, nodes_out_dev, n_nodes_out_dev,
                    result_out_dev, halton_next_out_dev, meta);
  if (r) return r;
  if (e->sampler_dubins)  // one row per step, recomputed from the nodes' library entries
    drlgx_launch_em_leaves_dubins(e->stream, n_sel, env_sel_dev, max_tree_nodes, e->S.A_max, e->S.cfg.angle_weight, e->tree_act, e->tree_link,
                                  e->tree_leaf, e->tree_meta, e->dubins, 1, nullptr, plan_out_dev, n_actions_out_dev, nullptr, nullptr);
  else
    drlgx_launch_em_leaves(e->stream, n_sel, env_sel_dev, max_tree_nodes, e->S.A_max, e->tree_act, e->tree_link, e->tree_leaf, e->tree_meta, 1,
                           nullptr, plan_out_dev, n_actions_out_dev);
  return check_launch(e);
}

int drlgx_stage_set_prior_information_host(drlgx_engine *e, int env, const double *information9) {
  DRLGX_ENTER(e);
  if (!e || env < 0 || env >= e->S.n_envs || !information9) return DRLGX_E_INVALID;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < r; ++c)
      if (information9[3 * r + c] != information9[3 * c + r]) return DRLGX_E_INVALID;  // symmetric, as an information matrix is
  HIPCHK(e, hipMemcpyAsync(e->S.prior + (size_t)env * DRLGX_PRIOR_STRIDE + 4, information9, 9 * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return DRLGX_OK;
}

int drlgx_stage_set_prior_pose_host(drlgx_engine *e, int env, const double *xytheta) {
  DRLGX_ENTER(e);
  if (!e || env < 0 || env >= e->S.n_envs || !xytheta) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  // (between the staged reset and the first measurement: one pose, no factor)
  int cnt[DRLGX_CNT_STRIDE];
  HIPCHK(e, hipMemcpyAsync(cnt, S.cnt + (size_t)env * DRLGX_CNT_STRIDE, sizeof(cnt), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (cnt[C_P] != 1 || cnt[C_M] != 0) return DRLGX_E_INVALID;
  const double p4[4] = {xytheta[0], xytheta[1], std::cos(xytheta[2]), std::sin(xytheta[2])};
  HIPCHK(e, hipMemcpyAsync(S.prior + (size_t)env * DRLGX_PRIOR_STRIDE, p4, sizeof(p4), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(S.th_pose + (size_t)env * S.P_max * 4, p4, sizeof(p4), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(S.est_pose + (size_t)env * S.P_max * 4, p4, sizeof(p4), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return DRLGX_OK;
}

int drlgx_set_fixed_landmarks_host(drlgx_engine *e, int n_fixed, const double *xy) {
  DRLGX_ENTER(e);
  if (!e || n_fixed < 0 || n_fixed > e->S.cfg.num_landmarks || (n_fixed > 0 && !xy)) return DRLGX_E_INVALID;
  if (!e->fixed_lm_dev) {
    int r = dev_alloc(e, &e->fixed_lm_dev, (size_t)std::max(e->S.cfg.num_landmarks, 1) * 2);
    if (r) return r;
  }
  if (n_fixed > 0) {
    HIPCHK(e, hipMemcpyAsync(e->fixed_lm_dev, xy, (size_t)n_fixed * 2 * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (the host buffer is the caller's)
  }
  e->S.fixed_lm = n_fixed > 0 ? e->fixed_lm_dev : nullptr;  // (the state struct travels with every launch: the next reset sees it)
  e->S.n_fixed = n_fixed;
  return DRLGX_OK;
}

int drlgx_set_planner_parameter(drlgx_engine *e, double angle_weight, double distance_weight0, double distance_weight1,
                                double occupancy_threshold, double max_edge_length, int algorithm) {
  DRLGX_ENTER(e);
  if (!e || !(max_edge_length > 0) || algorithm < 0 || algorithm > 3) return DRLGX_E_INVALID;
  drlgx_config &c = e->S.cfg;  // (the state struct is passed to every launch by value: the next launch sees the new values)
  c.angle_weight = angle_weight;
  c.distance_weight0 = distance_weight0;
  c.distance_weight1 = distance_weight1;
  c.occupancy_threshold = occupancy_threshold;
  c.max_edge_length = max_edge_length;
  c.algorithm = algorithm;
  return DRLGX_OK;
}

int drlgx_utility(drlgx_engine *e, const double *dist_dev, double *out_dev) {
  DRLGX_ENTER(e);
  if (!e || !out_dev) return DRLGX_E_INVALID;
  drlgx_launch_utility(e->S, e->stream, dist_dev, out_dev, 0);
  return check_launch(e);
}
int drlgx_uncertainty_em(drlgx_engine *e, int algorithm, double *out_dev) {
  DRLGX_ENTER(e);
  if (!e || !out_dev || (algorithm != DRLGX_ALG_EM_AOPT && algorithm != DRLGX_ALG_EM_DOPT)) return DRLGX_E_INVALID;
  drlgx_launch_utility(e->S, e->stream, nullptr, out_dev, algorithm == DRLGX_ALG_EM_DOPT ? 3 : 2);
  return check_launch(e);
}
int drlgx_explored(drlgx_engine *e, double *out_dev) {
  DRLGX_ENTER(e);
  if (!e || !out_dev) return DRLGX_E_INVALID;
  drlgx_launch_utility(e->S, e->stream, nullptr, out_dev, 1);
  return check_launch(e);
}

int drlgx_metrics(drlgx_engine *e, double sigma0, double *out_dev) {
  DRLGX_ENTER(e);
  if (!e || !out_dev) return DRLGX_E_INVALID;
  drlgx_launch_metrics(e->S, e->stream, sigma0, out_dev);
  return check_launch(e);
}
int drlgx_cov_array(drlgx_engine *e, double *length_dev, double *angle_dev) {
  DRLGX_ENTER(e);
  if (!e || !length_dev || !angle_dev) return DRLGX_E_INVALID;
  drlgx_launch_cov_array(e->S, e->stream, length_dev, angle_dev);
  return check_launch(e);
}

int drlgx_line_plan(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *goal_dev,
                    double *actions_dev, int32_t *n_actions_dev) {
  DRLGX_ENTER(e);
  if (!e || n_cand < 0 || !cand_env_dev || !goal_dev || !actions_dev || !n_actions_dev) return DRLGX_E_INVALID;
  if (n_cand == 0) return DRLGX_OK;
  drlgx_launch_line_plan(e->S, e->stream, n_cand, cand_env_dev, goal_dev, actions_dev, n_actions_dev);
  return check_launch(e);
}

int drlgx_lookahead(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev,
                    const int32_t *n_actions_dev, double *rewards_dev) {
  if (!e) return DRLGX_E_INVALID;
  return drlgx_lookahead_bounded(e, n_cand, cand_env_dev, actions_dev, n_actions_dev, e->S.A_max, rewards_dev);
}

int drlgx_lookahead_bounded(drlgx_engine *e, int n_cand, const int32_t *cand_env_dev, const double *actions_dev,
                            const int32_t *n_actions_dev, int max_n_actions, double *rewards_dev) {
  DRLGX_ENTER(e);
  if (!e || n_cand < 0 || !cand_env_dev || !actions_dev || !n_actions_dev || !rewards_dev || max_n_actions < 1 ||
      max_n_actions > e->S.A_max)
    return DRLGX_E_INVALID;
  if (n_cand == 0) return DRLGX_OK;
  if (e->S.n_roll < 1) return DRLGX_E_CAPACITY;
  const DrlgxState &S = e->S;
  const int base0 = S.n_envs, roll0 = 2 * S.n_envs;
  const int pbe = max_bound(e);  // rollouts start from their env's trajectory and add one pose per action
  {
    ScopedTimer t(e, 3);
    // deep copy env -> base, SLAM2D::set_copy_isam (re-base at the best estimate + one batch update)
    drlgx_launch_copy(e->fields_dev, (int)e->fields.size(), e->stream, S.n_envs, nullptr, nullptr, 0, base0, 3, e->S.cnt);
    drlgx_launch_rebase(S, e->stream, base0, S.n_envs);
  }
  {
    ScopedTimer t(e, 1);
    drlgx_launch_slam(S, e->stream, LaunchSel{base0, S.n_envs, nullptr, nullptr, 0}, pbe);
  }
  // candidates beyond the rollout capacity are processed in successive waves over the same rollout instances
  for (int c0 = 0; c0 < n_cand; c0 += S.n_roll) {
    const int nc = std::min(S.n_roll, n_cand - c0);
    const int32_t *ce = cand_env_dev + c0;
    const double *act = actions_dev + (size_t)c0 * S.A_max * 3;
    const int32_t *na = n_actions_dev + c0;
    {
      ScopedTimer t(e, 3);
      drlgx_launch_copy(e->fields_dev, (int)e->fields.size(), e->stream, nc, ce, nullptr, base0, roll0, 3, e->S.cnt,
                        &S);  // (with the base solve's covariance panel)
      drlgx_launch_fix_rollouts(S, e->stream, nc, ce, roll0);
    }
    // whole action lists per launch where the loop kernels serve them, one launch per action index from a_begin on
    LaunchSel sel{roll0, nc, nullptr, na, 0};
    sel.map_last_only = 1;
    const int a_begin = launch_action_range(e, sel, act, 1, pbe, max_n_actions, true, true);
    for (int a = a_begin; a < max_n_actions; ++a) {
      sel.act_idx = a;
      launch_belief_step(e, sel, act, S.A_max * 3, 1, std::min(pbe + a + 1, S.P_max), false);
    }
    drlgx_launch_rewards(S, e->stream, nc, ce, roll0, rewards_dev + c0);
  }
  return check_launch(e);
}

// ---- graph export ------------------------------------------------------------------------------
int drlgx_graph_capacity(const drlgx_engine *e, int *max_nodes, int *max_edges, int *max_frontier) {
  if (!e) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  if (max_nodes) *max_nodes = S.n_envs * (2 * S.L_max + S.P_max + 1);
  if (max_edges) *max_edges = S.n_envs * 2 * (S.M_max + S.P_max + S.L_max + 1);
  if (max_frontier) *max_frontier = S.L_max + 1;
  return DRLGX_OK;
}

int drlgx_graph(drlgx_engine *e, int32_t *node_off_dev, int32_t *edge_off_dev, float *x_dev, int64_t *edge_index_dev,
                float *edge_attr_dev, int32_t *n_frontier_dev, double *frontier_xy_dev, int32_t *nearest_frontier_node_dev) {
  DRLGX_ENTER(e);
  if (!e || !node_off_dev || !edge_off_dev || !x_dev || !edge_index_dev || !edge_attr_dev || !n_frontier_dev ||
      !frontier_xy_dev || !nearest_frontier_node_dev)
    return DRLGX_E_INVALID;
  ScopedTimer t(e, 4);
  drlgx_launch_graph(e->S, e->stream, e->graph_gi, e->graph_gi_stride, node_off_dev, edge_off_dev, x_dev, edge_index_dev,
                     edge_attr_dev, n_frontier_dev, frontier_xy_dev, nearest_frontier_node_dev, e->S.L_max + 1);
  return check_launch(e);
}

// ---- getters -----------------------------------------------------------------------------------
static int fetch(drlgx_engine *e, void *dst, const void *src, size_t bytes) {
  HIPCHK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
  return DRLGX_OK;
}
#define INST_OK(e, inst) ((e) && (inst) >= 0 && (inst) < (e)->S.n_inst)

int drlgx_get_counts_host(drlgx_engine *e, int inst, int32_t out[5]) {
  DRLGX_ENTER(e);
  if (!INST_OK(e, inst) || !out) return DRLGX_E_INVALID;
  int c[DRLGX_CNT_STRIDE];
  int r = fetch(e, c, e->S.cnt + (size_t)inst * DRLGX_CNT_STRIDE, sizeof(c));
  if (r) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  out[0] = c[C_P]; out[1] = c[C_L]; out[2] = c[C_M]; out[3] = c[C_STEP]; out[4] = c[C_ISAM];
  return DRLGX_OK;
}

int drlgx_counts(drlgx_engine *e, int32_t *counts_dev) {
  DRLGX_ENTER(e);
  if (!e || !counts_dev) return DRLGX_E_INVALID;
  HIPCHK(e, hipMemcpy2DAsync(counts_dev, 5 * sizeof(int32_t), e->S.cnt, DRLGX_CNT_STRIDE * sizeof(int32_t), 5 * sizeof(int32_t),
                             (size_t)e->S.n_envs, hipMemcpyDeviceToDevice, e->stream));
  return DRLGX_OK;
}

int drlgx_get_poses_host(drlgx_engine *e, int inst, double *xytheta, double *information) {
  DRLGX_ENTER(e);
  int32_t c[5];
  int r = drlgx_get_counts_host(e, inst, c);
  if (r) return r;
  const DrlgxState &S = e->S;
  const int P = c[0];
  std::vector<double> ep((size_t)P * 4), pi((size_t)P * 6);
  if ((r = fetch(e, ep.data(), S.est_pose + (size_t)inst * S.P_max * 4, ep.size() * 8))) return r;
  if ((r = fetch(e, pi.data(), S.pose_info + (size_t)inst * S.P_max * 6, pi.size() * 8))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (int i = 0; i < P; ++i) {
    if (xytheta) {
      xytheta[3 * i] = ep[4 * i];
      xytheta[3 * i + 1] = ep[4 * i + 1];
      xytheta[3 * i + 2] = std::atan2(ep[4 * i + 3], ep[4 * i + 2]);
    }
    if (information) {
      const double *s = &pi[6 * i];
      double *o = information + 9 * i;
      o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
      o[3] = s[1]; o[4] = s[3]; o[5] = s[4];
      o[6] = s[2]; o[7] = s[4]; o[8] = s[5];
    }
  }
  return DRLGX_OK;
}

static int sorted_slots(drlgx_engine *e, int inst, int L, std::vector<int> &keys, std::vector<int> &order) {
  const DrlgxState &S = e->S;
  keys.resize(L);
  int r = fetch(e, keys.data(), S.lm_key + (size_t)inst * S.L_max, (size_t)L * sizeof(int));
  if (r) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  order.resize(L);
  for (int j = 0; j < L; ++j) order[j] = j;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return keys[a] < keys[b]; });
  return DRLGX_OK;
}

int drlgx_get_landmarks_host(drlgx_engine *e, int inst, int32_t *keys, double *xy, double *information) {
  DRLGX_ENTER(e);
  int32_t c[5];
  int r = drlgx_get_counts_host(e, inst, c);
  if (r) return r;
  const DrlgxState &S = e->S;
  const int L = c[1];
  std::vector<int> k, ord;
  if ((r = sorted_slots(e, inst, L, k, ord))) return r;
  std::vector<double> el((size_t)L * 2), li((size_t)L * 3);
  if ((r = fetch(e, el.data(), S.est_lm + (size_t)inst * S.L_max * 2, el.size() * 8))) return r;
  if ((r = fetch(e, li.data(), S.lm_info + (size_t)inst * S.L_max * 3, li.size() * 8))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (int n = 0; n < L; ++n) {
    int j = ord[n];
    if (keys) keys[n] = k[j];
    if (xy) {
      xy[2 * n] = el[2 * j];
      xy[2 * n + 1] = el[2 * j + 1];
    }
    if (information) {
      information[4 * n] = li[3 * j];
      information[4 * n + 1] = li[3 * j + 1];
      information[4 * n + 2] = li[3 * j + 1];
      information[4 * n + 3] = li[3 * j + 2];
    }
  }
  return DRLGX_OK;
}

int drlgx_get_cov_traces_host(drlgx_engine *e, int inst, double *lm_trace, double *pose_trace) {
  DRLGX_ENTER(e);
  int32_t c[5];
  int r = drlgx_get_counts_host(e, inst, c);
  if (r) return r;
  const DrlgxState &S = e->S;
  const int P = c[0], L = c[1];
  std::vector<int> k, ord;
  if ((r = sorted_slots(e, inst, L, k, ord))) return r;
  std::vector<double> lt(L), pt(P);
  if ((r = fetch(e, lt.data(), S.lm_tr + (size_t)inst * S.L_max, (size_t)L * 8))) return r;
  if ((r = fetch(e, pt.data(), S.pose_tr + (size_t)inst * S.P_max, (size_t)P * 8))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (lm_trace)
    for (int n = 0; n < L; ++n) lm_trace[n] = lt[ord[n]];
  if (pose_trace)
    for (int i = 0; i < P; ++i) pose_trace[i] = pt[i];
  return DRLGX_OK;
}

int drlgx_debug_disc_cells_bound(double radius_cells) {
  if (!(radius_cells >= 0.0 && radius_cells <= 64.0)) return DRLGX_E_INVALID;
  return disc_cells_bound(radius_cells);
}

int drlgx_debug_map_compact_ok(const drlgx_engine *e, int p_bound) {
  if (!e) return DRLGX_E_INVALID;
  return drlgx_map_compact_ok(e->S, p_bound) ? 1 : 0;
}

int drlgx_vm_shape(const drlgx_engine *e, int *rows, int *cols) {
  if (!e) return DRLGX_E_INVALID;
  if (rows) *rows = e->S.rows;
  if (cols) *cols = e->S.cols;
  return DRLGX_OK;
}

int drlgx_get_virtual_map_host(drlgx_engine *e, int inst, double *prob, double *info, double *cov_trace,
                               uint8_t *updated) {
  DRLGX_ENTER(e);
  if (!INST_OK(e, inst)) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  const size_t V = S.V;
  std::vector<double> pl(3 * V);
  int r;
  if (prob && (r = fetch(e, prob, S.vm_prob + (size_t)inst * V, V * 8))) return r;
  if ((r = fetch(e, pl.data(), S.vm_info + (size_t)inst * 3 * V, 3 * V * 8))) return r;
  if (updated && (r = fetch(e, updated, S.vm_upd + (size_t)inst * S.Vu, V))) return r;
  if (cov_trace && (r = fetch(e, cov_trace, S.vm_tr + (size_t)inst * V, V * 8))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (info)
    for (size_t v = 0; v < V; ++v) {
      const double a = pl[v], b = pl[V + v], d = pl[2 * V + v];
      info[4 * v] = a; info[4 * v + 1] = b; info[4 * v + 2] = b; info[4 * v + 3] = d;
    }
  return DRLGX_OK;
}

int drlgx_get_ground_truth_host(drlgx_engine *e, int inst, double *vehicle_xytheta, double *landmarks_xy) {
  DRLGX_ENTER(e);
  if (!INST_OK(e, inst)) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  double gp[4];
  int parent = 0, r;
  if ((r = fetch(e, gp, S.gt_pose + (size_t)inst * 4, sizeof(gp)))) return r;
  if ((r = fetch(e, &parent, S.parent + inst, sizeof(int)))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (vehicle_xytheta) {
    vehicle_xytheta[0] = gp[0];
    vehicle_xytheta[1] = gp[1];
    vehicle_xytheta[2] = std::atan2(gp[3], gp[2]);
  }
  if (landmarks_xy && S.cfg.num_landmarks > 0) {
    if ((r = fetch(e, landmarks_xy, S.gt_lm + (size_t)parent * S.LG * 2, (size_t)S.cfg.num_landmarks * 2 * 8))) return r;
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  return DRLGX_OK;
}

int drlgx_get_factors_host(drlgx_engine *e, int inst, int32_t *pose, int32_t *key, double *bearing, double *range) {
  DRLGX_ENTER(e);
  int32_t c[5];
  int r = drlgx_get_counts_host(e, inst, c);
  if (r) return r;
  const DrlgxState &S = e->S;
  const int L = c[1], M = c[2];
  std::vector<int> keys(L), mp(M), ml(M);
  std::vector<double> br((size_t)M * 2);
  if ((r = fetch(e, keys.data(), S.lm_key + (size_t)inst * S.L_max, (size_t)L * 4))) return r;
  if ((r = fetch(e, mp.data(), S.meas_pose + (size_t)inst * S.M_max, (size_t)M * 4))) return r;
  if ((r = fetch(e, ml.data(), S.meas_lm + (size_t)inst * S.M_max, (size_t)M * 4))) return r;
  if ((r = fetch(e, br.data(), S.meas_br + (size_t)inst * S.M_max * 2, (size_t)M * 16))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (int m = 0; m < M; ++m) {
    if (pose) pose[m] = mp[m];
    if (key) key[m] = keys[ml[m]];
    if (bearing) bearing[m] = br[2 * m];
    if (range) range[m] = br[2 * m + 1];
  }
  return DRLGX_OK;
}

// SLAM2D::adjacency_degree_get (SLAM2D.cpp:198-273) assembled from the exported factor list.
int drlgx_get_adjacency_host(drlgx_engine *e, int inst, double *adjacency, double *features) {
  DRLGX_ENTER(e);
  int32_t c[5];
  int r = drlgx_get_counts_host(e, inst, c);
  if (r) return r;
  const DrlgxState &S = e->S;
  const int P = c[0], L = c[1], M = c[2], N = P + L;
  std::vector<int> k, ord;
  if ((r = sorted_slots(e, inst, L, k, ord))) return r;
  std::vector<int> node_of_slot(L);
  for (int n = 0; n < L; ++n) node_of_slot[ord[n]] = n;
  std::vector<int> mp(M), ml(M);
  std::vector<double> br((size_t)M * 2), odo((size_t)P * 4), lt(L), pt(P);
  if ((r = fetch(e, mp.data(), S.meas_pose + (size_t)inst * S.M_max, (size_t)M * 4))) return r;
  if ((r = fetch(e, ml.data(), S.meas_lm + (size_t)inst * S.M_max, (size_t)M * 4))) return r;
  if ((r = fetch(e, br.data(), S.meas_br + (size_t)inst * S.M_max * 2, (size_t)M * 16))) return r;
  if ((r = fetch(e, odo.data(), S.odo + (size_t)inst * S.P_max * 4, (size_t)P * 32))) return r;
  if ((r = fetch(e, lt.data(), S.lm_tr + (size_t)inst * S.L_max, (size_t)L * 8))) return r;
  if ((r = fetch(e, pt.data(), S.pose_tr + (size_t)inst * S.P_max, (size_t)P * 8))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (adjacency) std::fill(adjacency, adjacency + (size_t)N * N, 0.0);
  if (features) std::fill(features, features + N, 0.0);
  for (int i = 0; i + 1 < P; ++i) {
    double d = std::sqrt(std::pow(odo[4 * i], 2) + std::pow(odo[4 * i + 1], 2)) + 0.001;
    int a = L + i, b = L + i + 1;
    if (adjacency) adjacency[(size_t)a * N + b] = adjacency[(size_t)b * N + a] = d;
    if (features) {
      features[a] = pt[i];
      features[b] = pt[i + 1];
    }
  }
  for (int m = 0; m < M; ++m) {
    int a = L + mp[m], b = node_of_slot[ml[m]];
    if (adjacency) adjacency[(size_t)a * N + b] = adjacency[(size_t)b * N + a] = br[2 * m + 1];
    if (features) {
      features[a] = pt[mp[m]];
      features[b] = lt[ml[m]];
    }
  }
  return DRLGX_OK;
}

int drlgx_get_landmark_order_host(const drlgx_engine *e, int32_t *order) {
  if (!e || !order) return DRLGX_E_INVALID;
  for (int i = 0; i < e->S.cfg.num_landmarks; ++i) order[i] = e->lm_order[i];
  return DRLGX_OK;
}

// ---- snapshots ---------------------------------------------------------------------------------
// Snapshots are extra instances in the same HBM arrays: one copy kernel moves every field.
int drlgx_snapshot(drlgx_engine *e, int slot) {
  DRLGX_ENTER(e);
  if (!e || slot < 0 || slot >= e->S.cfg.max_snapshots) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  ScopedTimer t(e, 3);
  drlgx_launch_copy(e->fields_dev, (int)e->fields.size(), e->stream, S.n_envs, nullptr, nullptr, 0, snapshot_base(e, slot), 0, e->S.cnt, &S);
  e->snap_pbound[slot] = e->pbound;
  return check_launch(e);
}

static bool restore_is_compact(const drlgx_engine *e) {
  return e->restore_compact && !e->restore_eager && (int)e->restore_tab.size() <= kRestoreMaxEntries;
}

int drlgx_restore(drlgx_engine *e, int slot) {
  DRLGX_ENTER_OWING(e);  // (a debt of an earlier restore is void: this one replaces every plane it covered)
  if (!e || slot < 0 || slot >= e->S.cfg.max_snapshots) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  ScopedTimer t(e, 3);
  // lazy: everything but the virtual-map planes (43 % of an instance's live bytes at the bench state), which the next belief step
  // rebuilds without reading them, and the bodies of the valid covariance panels, which it reads where they are - or settle() copies
  // both before anything else touches the envs
  // (the lazy form by one workgroup per env over its own table, k_restore_compact; the generic kernel's is the A/B)
  if (restore_is_compact(e))
    drlgx_launch_restore_compact(e->restore_tab_dev, (int)e->restore_tab.size(), e->restore_n16, e->stream, S.n_envs, snapshot_base(e, slot),
                                 S.cnt, S.jc ? S.jc_meta : nullptr);
  else
    drlgx_launch_copy(e->fields_dev, (int)e->fields.size(), e->stream, S.n_envs, nullptr, nullptr, snapshot_base(e, slot), 0,
                      e->restore_eager ? 0 : 1, e->S.cnt, &S, -1, e->restore_eager ? 1 : 2);
  e->owed_slot = e->restore_eager ? -1 : slot;
  e->pbound = e->snap_pbound[slot];
  return check_launch(e);
}

// ---- development aid: in-kernel phase stamps of block 0 ------------------------------------------
int drlgx_debug_phase_clocks_host(drlgx_engine *e, int arm, int64_t out[64]) {
  DRLGX_ENTER(e);
  if (!e) return DRLGX_E_INVALID;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->S.prof_block = (arm >> 8) & 0xffff;  // (arm >> 8: the workgroup whose phases are stamped; 0 by default)
  // (arm & 2: the second bank of 64 stamps - per-wave stamps of one sweep block step)
  // (arm & 4: 1024 stamps - out must hold them: banks 0, 1 and the per-workgroup start / end stamps of k_step from 128 on)
  // (arm & 4 reads the whole buffer from its start, whatever arm & 2 says: the buffer holds exactly 1024 stamps)
  if (out && e->S.prof)
    HIPCHK(e, hipMemcpy(out, e->S.prof + ((arm & 4) ? 0 : ((arm & 2) ? 64 : 0)), ((arm & 4) ? 1024 : 64) * sizeof(long long), hipMemcpyDeviceToHost));
  if (arm && !e->S.prof) {
    long long *p = nullptr;
    int r = dev_alloc(e, &p, 1024);
    if (r) return r;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->S.prof = p;
  } else if (!arm) {
    e->S.prof = nullptr;
  }
  return DRLGX_OK;
}

// ---- incremental belief update: how many SLAM updates took the rank-k path / the full solve ------------------
int drlgx_inc_stats_host(drlgx_engine *e, int64_t out[2], int reset) {
  DRLGX_ENTER_OWING(e);
  if (!e || !out) return DRLGX_E_INVALID;
  out[0] = out[1] = -1;  // -1: the incremental path is disabled (DRLGX_INCREMENTAL=0 or the panels exceed the memory budget)
  if (!e->S.inc_stats) return DRLGX_OK;
  unsigned long long v[2] = {0, 0};
  HIPCHK(e, hipMemcpyAsync(v, e->S.inc_stats, sizeof(v), hipMemcpyDeviceToHost, e->stream));
  if (reset) HIPCHK(e, hipMemsetAsync(e->S.inc_stats, 0, sizeof(v), e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  out[0] = (int64_t)v[0];
  out[1] = (int64_t)v[1];
  return DRLGX_OK;
}

// ---- development aid: the covariance panel of one instance (env, look-ahead copy or snapshot) --------------------
int drlgx_debug_panel_host(drlgx_engine *e, int inst, int32_t meta[4], double *panel, size_t panel_cap) {
  DRLGX_ENTER(e);  // (reads a panel: whatever a lazy restore owes is settled first)
  if (!INST_OK(e, inst) || !meta) return DRLGX_E_INVALID;
  const DrlgxState &S = e->S;
  meta[0] = meta[1] = meta[2] = meta[3] = 0;
  if (!S.jc) return DRLGX_OK;
  int r = fetch(e, meta, S.jc_meta + (size_t)inst * 4, 4 * sizeof(int32_t));
  if (r) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (!panel || meta[0] != 1) return DRLGX_OK;
  const int P = meta[1], L = meta[2];
  if (P < 0 || P > S.P_max || L < 0 || L > S.L_max) return DRLGX_E_INVALID;
  const size_t cols = 3 + 2 * (size_t)L, rows = 3 * (size_t)P + 2 * (size_t)L;
  if (rows * cols > panel_cap) return DRLGX_E_INVALID;
  const double *src = S.jc + (size_t)inst * S.jc_stride;
  // the pose rows, then the landmark rows (which start at row 3 P_max of the instance's panel)
  if (P > 0) HIPCHK(e, hipMemcpy2DAsync(panel, cols * 8, src, (size_t)S.jc_ld * 8, cols * 8, 3 * (size_t)P, hipMemcpyDeviceToHost, e->stream));
  if (L > 0)
    HIPCHK(e, hipMemcpy2DAsync(panel + 3 * (size_t)P * cols, cols * 8, src + 3 * (size_t)S.P_max * S.jc_ld, (size_t)S.jc_ld * 8, cols * 8,
                               2 * (size_t)L, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return DRLGX_OK;
}

// ---- development aid: the compact restore's table ----------------------------------------------------------------
int drlgx_debug_restore_table_host(const drlgx_engine *e, int32_t info[4], int64_t *rows, int rows_cap) {
  if (!e || !info) return DRLGX_E_INVALID;
  const int n = (int)e->restore_tab.size();
  info[0] = n;
  info[1] = e->restore_n16;
  info[2] = restore_is_compact(e) ? 1 : 0;
  info[3] = drlgx_restore_items_per_trip();
  for (int k = 0; rows && k < n && k < rows_cap; ++k) {
    const DrlgxField &f = e->restore_tab[k];
    rows[4 * k] = (int64_t)f.stride;
    rows[4 * k + 1] = f.unit;
    rows[4 * k + 2] = f.unit_bytes;
    rows[4 * k + 3] = f.pad;
  }
  return DRLGX_OK;
}

int64_t drlgx_debug_field_live_bytes(int64_t stride, int unit, int unit_bytes, int pad, int count) {
  if (stride < 0 || unit < 0 || unit_bytes < 0) return -1;
  return (int64_t)drlgx_field_live_bytes((size_t)stride, unit, unit_bytes, pad, count);
}

// ---- timing ------------------------------------------------------------------------------------
int drlgx_timing_enable(drlgx_engine *e, int on) {
  DRLGX_ENTER_OWING(e);
  if (!e) return DRLGX_E_INVALID;
  e->timing = on != 0;
  e->per_stage = on == 2;
  return DRLGX_OK;
}

int drlgx_timing_read_host(drlgx_engine *e, double ms[DRLGX_N_TIMERS], int64_t launches[DRLGX_N_TIMERS]) {
  DRLGX_ENTER_OWING(e);
  if (!e) return DRLGX_E_INVALID;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (auto &sp : e->spans) {
    float t = 0;
    if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess && sp.id >= 0 && sp.id < DRLGX_N_TIMERS) {
      e->t_ms[sp.id] += t;
      e->t_n[sp.id] += 1;
    }
    e->free_events.push_back(sp.a);
    e->free_events.push_back(sp.b);
  }
  e->spans.clear();
  for (int i = 0; i < DRLGX_N_TIMERS; ++i) {
    if (ms) ms[i] = e->t_ms[i];
    if (launches) launches[i] = e->t_n[i];
    e->t_ms[i] = 0;
    e->t_n[i] = 0;
  }
  return DRLGX_OK;
}

}  // extern "C"
