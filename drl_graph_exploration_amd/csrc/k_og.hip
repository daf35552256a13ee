// Expected map entropy of candidate plans: calculateUncertainty_OG_SHANNON (src/em_exploration/Planner2D.cpp:368-392) for action
// lists the caller supplies -
//   node->virtual_map->updateProbability(slam, sensor_model)   (VirtualMap.cpp:61-84: OccupancyMap::update(map), OccupancyMap.cpp:122-138)
//   uncertainty = sum_v -p_v ln p_v - (1 - p_v) ln(1 - p_v)     (:383-389)
//   node->cost = uncertainty + distance * distance_weight_      (:418-420, :1322-1332)
// without simulating, without noise, without re-solving and without any covariance: the leaf's map holds the P old poses at the
// current estimate and one pose per action at the noise-free predicted pose chained from the last estimate (kem::leaf_pose), and
// the landmarks at their current estimates.  The occupancy grid is rebuilt from the untouched map: the landmarks' cells, then
// every pose in trajectory order.  Nothing of the live environment is written.
//
// One workgroup per candidate.  The P + K poses (x y c s) and their bounding boxes are staged in LDS once, the landmarks as the
// count per cell.  The cell pass is cell-centric: a wave takes an 8 x 8 tile of cells, a lane walks the poses in trajectory order
// for its cell and steps the ladder's state machine (kmap::LadderFsm, the packed tables of DrlgxState::lo_tocc ...) at every pose
// that sees it - the order matters once the ladder clamps, so there is no mask and no pose-centric pass; a cell whose state maps
// to itself stops early, as in kmap::cell_pass.  The two sums are reduced within a wave, then across the waves through LDS in
// wave order: repeated calls give the same bits.  Part of the k_step.hip unity build: kmap's and kem's device functions as they
// are, and -ffp-contract=off for the gates.
#include "drlgx_dev.h"

namespace kog {

constexpr int kT = kmap::kThreads;  // (kmap::bbox_sweep deals its (pose, sample) pairs to a workgroup of this size)
constexpr int kWaves = kT / 64;

// doubles: poses [cap][4] | sums of the waves [2][kWaves] | the plan's distance | ladder values [DRLGX_LO_TAB];
// ints: bbox [cap][4] | landmarks per cell [V]
__host__ __device__ inline size_t lds_bytes(int cap, int V) {
  return ((size_t)cap * 4 + 2 * kWaves + 1 + DRLGX_LO_TAB) * sizeof(double) + ((size_t)cap * 4 + (size_t)V) * sizeof(int);
}

// What k_og_cost could only report through the status word, found out before it is launched: a candidate that names no environment
// or has more actions than max_actions.  flag[0] = DRLGX_E_INVALID then (the caller zeroes it).
__global__ void k_og_check(DRLGX_KS_PARAM, int n_cand, const int32_t *cand_env, const int32_t *n_actions, int *flag) {
  const DrlgxState &S = DRLGX_KS_REF;
  const int ci = blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= n_cand) return;
  const int env = cand_env[ci], K = n_actions[ci];
  if (env < 0 || env >= S.n_envs || K < 0 || K > S.A_max) atomicMin(flag, DRLGX_E_INVALID);
}

// cand_env / actions / n_actions: [gridDim.x] candidates in drlgx_em_cost's layout; ent_out / cost_out [gridDim.x], prob_out
// [gridDim.x][V], dist_out [gridDim.x][2] (the two factors of the cost's second term: the plan's distance, the distance weight), any
// of them null
__global__ __launch_bounds__(kT) void k_og_cost(DRLGX_KS_PARAM, const int32_t *cand_env, const double *actions, const int32_t *n_actions,
                                                double *ent_out, double *cost_out, double *prob_out, double *dist_out) {
  const DrlgxState &S = DRLGX_KS_REF;
  extern __shared__ __attribute__((aligned(16))) double og_smem[];
  const drlgx_config &cfg = S.cfg;
  const int tid = drlgx_tid(), lane = tid & 63, wave = tid >> 6, ci = blockIdx.x;
  const int env = cand_env[ci];
  const int K = n_actions[ci];
  const bool env_ok = env >= 0 && env < S.n_envs;
  const int P = env_ok ? S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_P] : 0, L = env_ok ? S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_L] : 0;
  const int cap = S.P_max + S.A_max, np = P + K, V = S.V;
  if (!env_ok || K < 0 || K > S.A_max || P < 1 || P > S.P_max || L < 0 || L > S.L_max) {  // (the host checked: flag it, touch nothing)
    if (tid == 0) atomicMin(S.status, DRLGX_E_CAPACITY);
    return;
  }
  kmap::MapCtx c;  // (what kmap::bbox_sweep reads: the pose table, the boxes, the pose count)
  c.sp = og_smem;
  double *red = c.sp + (size_t)cap * 4, *sdist = red + 2 * kWaves, *lpv = sdist + 1;
  c.bbox = reinterpret_cast<int *>(lpv + DRLGX_LO_TAB);
  c.P = np;
  int *lmc = c.bbox + (size_t)cap * 4;
  const double *ep = S.est_pose + (size_t)env * S.P_max * 4;
  const double *el = S.est_lm + (size_t)env * S.L_max * 2;
  const double *act = actions + (size_t)ci * S.A_max * 3;

  // ---- staging: one lane per pose (the first lanes), the plan's distance on the last one; the cells' landmark counts cleared ----
  for (int i = tid; i < np; i += kT) {
    const Pose ps = kem::leaf_pose(ep, P, act, i);
    c.sp[4 * i] = ps.x; c.sp[4 * i + 1] = ps.y; c.sp[4 * i + 2] = ps.c; c.sp[4 * i + 3] = ps.s;
    kmap::bbox_origin(S, c.bbox + 4 * i, ps.x, ps.y);
  }
  if (tid == kT - 1) *sdist = kem::plan_distance(cfg, act, K);
  if (tid < S.lo_ntab) lpv[tid] = S.lo_pv[tid];  // (lo_ntab <= DRLGX_LO_TAB < kT)
  for (int v = tid; v < V; v += kT) lmc[v] = 0;
  __syncthreads();
  // every estimated landmark inside the grid is one occupied update of its cell (OccupancyMap.cpp:127-131)
  for (int j = tid; j < L; j += kT) {
    const int v = kmap::landmark_cell(S, el[2 * j], el[2 * j + 1]);
    if (v >= 0) atomicAdd(&lmc[v], 1);
  }
  const bool use_bbox = !S.bbox_noop;  // (else the box provably holds every in-range cell: k_map.hip)
  if (use_bbox) kmap::bbox_sweep(S, c);
  __syncthreads();

  // ---- cell pass: one 8 x 8 tile of cells per wave and round (lane = 8 (row mod 8) + (col mod 8), as kmap::cell_pass) ----
  const int cols = S.cols, rows = S.rows;
  const int tiles_c = (cols + 7) >> 3, ntiles = ((rows + 7) >> 3) * tiles_c;
  const kmap::LadderFsm fsm{S.lo_tocc, S.lo_tfree, S.lo_tflag};
  const double *live = S.vm_prob + (size_t)env * V;
  double *pout = prob_out ? prob_out + (size_t)ci * V : nullptr;
  double s_h = 0.0, s_known = 0.0;
  for (int t = wave; t < ntiles; t += kWaves) {
    const int trow = t / tiles_c, tcol = t - trow * tiles_c;
    const int row = 8 * trow + (lane >> 3), col = 8 * tcol + (lane & 7);
    if (!(row < rows && col < cols)) continue;
    const int v = row * cols + col;
    const P2 pt = kmap::cell_centre(cfg, row, col);
    int st = 0;  // LOGODDS_UNKNOWN
    for (int n = lmc[v]; n > 0; --n) st = fsm.landmark(st);
    for (int i = 0; i < np; ++i) {
      // OccupancyMap::update(state) (OccupancyMap.cpp:98-118): the cell lies in the pose's box and passes checkWithoutMinRange
      if (use_bbox && (row < c.bbox[4 * i] || row > c.bbox[4 * i + 1] || col < c.bbox[4 * i + 2] || col > c.bbox[4 * i + 3])) continue;
      const Pose ps{c.sp[4 * i], c.sp[4 * i + 1], c.sp[4 * i + 2], c.sp[4 * i + 3]};
      const double gx = ps.x - pt.x, gy = ps.y - pt.y;
      if (!(gx * gx + gy * gy < S.r2_max_lt)) continue;  // sqrt(d2) < max_range, exactly
      if (!kmap::in_fov(S, ps, pt)) continue;
      const int nst = fsm.seen(st);
      if (nst == st) break;  // absorbing: the transition depends on the state only
      st = nst;
    }
    const double pv = lpv[st];  // VirtualMap::updateProbability: the host's value table
    if (pout) pout[v] = pv;
    s_h += -pv * log(pv) - (1.0 - pv) * log(1.0 - pv);
    if (live[v] < cfg.occupancy_threshold) s_known += 1.0;  // the LIVE map (Planner2D.cpp:1322-1325)
  }

  // ---- reductions: within a wave, then across the waves in wave order ----
  s_h = kmap::wave_sum63(s_h);
  s_known = kmap::wave_sum63(s_known);
  if (lane == 63) {
    red[wave] = s_h;
    red[kWaves + wave] = s_known;
  }
  __syncthreads();
  if (tid == 0) {
    double h = 0.0, known = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      h += red[w];
      known += red[kWaves + w];
    }
    if (ent_out) ent_out[ci] = h;
    if (cost_out || dist_out) {
      const double pk = known / (double)V;
      const double dw = cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * pk;
      if (cost_out) cost_out[ci] = h + *sdist * dw;
      if (dist_out) {
        dist_out[2 * ci] = *sdist;
        dist_out[2 * ci + 1] = dw;
      }
    }
  }
}

// ---- the leaves of a sampling tree (drlgx_og_plan): every leaf of a tree starts from the same landmarks and the same P old poses, so
// k_og_tree_base walks those once per environment and k_og_tree_cost walks a leaf's K new poses only.  The ladder is a state machine
// over the pose sequence: the state k_og_cost holds in `st` when it reaches pose index P is what the base leaves in its byte plane
// (a walk k_og_cost ended early at an old pose stands in a state that maps to itself: the leaf's walk ends at its first pose that
// sees the cell, in the same state).  The entropy term depends on the state only (a table built with k_og_cost's expression), the
// lanes add their tiles' terms in k_og_cost's order and the waves' sums meet in wave order: the same bits as k_og_cost.
//
// LDS of the base: doubles poses [P_max][4]; ints bbox [P_max][4] | landmarks per cell [V] | known cells of the waves [kWaves] (all
// dynamic: a static array on top of the 160 KB the launcher may ask for would make that request invalid).  Of a leaf: doubles poses [A_max][4] |
// sums of the waves [kWaves] | the plan's distance | entropy per ladder state [DRLGX_LO_TAB]; ints bbox [A_max][4].
__host__ __device__ inline size_t tree_base_lds_bytes(int P_max, int V) {
  return (size_t)P_max * 4 * sizeof(double) + ((size_t)P_max * 4 + (size_t)V + kWaves) * sizeof(int);
}
__host__ __device__ inline size_t tree_leaf_lds_bytes(int A_max) {
  return ((size_t)A_max * 4 + kWaves + 1 + DRLGX_LO_TAB) * sizeof(double) + (size_t)A_max * 4 * sizeof(int);
}

// One workgroup per selected environment.  base [n_envs][Vu] (row env_sel[blockIdx.x]): per cell the ladder state after the landmark
// updates and the P old poses; known [n_envs]: the cells of the LIVE map below the occupancy threshold (Planner2D.cpp:1322-1325) - a
// count, exact in any order.  An environment listed twice is written twice with the same values.
__global__ __launch_bounds__(kT) void k_og_tree_base(DRLGX_KS_PARAM, const int32_t *env_sel, uint8_t *base, int32_t *known) {
  const DrlgxState &S = DRLGX_KS_REF;
  extern __shared__ __attribute__((aligned(16))) double og_smem[];
  const drlgx_config &cfg = S.cfg;
  const int tid = drlgx_tid(), lane = tid & 63, wave = tid >> 6;
  const int env = env_sel[blockIdx.x];
  const bool env_ok = env >= 0 && env < S.n_envs;
  const int P = env_ok ? S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_P] : 0, L = env_ok ? S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_L] : 0;
  const int V = S.V;
  if (!env_ok || P < 1 || P > S.P_max || L < 0 || L > S.L_max) {  // (the tree's kernel refused such a call: flag it, touch nothing)
    if (tid == 0) atomicMin(S.status, DRLGX_E_CAPACITY);
    return;
  }
  kmap::MapCtx c;
  c.sp = og_smem;
  c.bbox = reinterpret_cast<int *>(c.sp + (size_t)S.P_max * 4);
  c.P = P;
  int *lmc = c.bbox + (size_t)S.P_max * 4, *kred = lmc + V;
  const double *ep = S.est_pose + (size_t)env * S.P_max * 4;
  const double *el = S.est_lm + (size_t)env * S.L_max * 2;
  for (int i = tid; i < P; i += kT) {
    const double x = ep[4 * i], y = ep[4 * i + 1];
    c.sp[4 * i] = x; c.sp[4 * i + 1] = y; c.sp[4 * i + 2] = ep[4 * i + 2]; c.sp[4 * i + 3] = ep[4 * i + 3];
    kmap::bbox_origin(S, c.bbox + 4 * i, x, y);
  }
  for (int v = tid; v < V; v += kT) lmc[v] = 0;
  __syncthreads();
  for (int j = tid; j < L; j += kT) {
    const int v = kmap::landmark_cell(S, el[2 * j], el[2 * j + 1]);
    if (v >= 0) atomicAdd(&lmc[v], 1);
  }
  const bool use_bbox = !S.bbox_noop;
  if (use_bbox) kmap::bbox_sweep(S, c);
  __syncthreads();

  const int cols = S.cols, rows = S.rows;
  const int tiles_c = (cols + 7) >> 3, ntiles = ((rows + 7) >> 3) * tiles_c;
  const kmap::LadderFsm fsm{S.lo_tocc, S.lo_tfree, S.lo_tflag};
  const double *live = S.vm_prob + (size_t)env * V;
  uint8_t *plane = base + (size_t)env * S.Vu;
  int n_known = 0;  // (of the wave: the same in every lane)
  for (int t = wave; t < ntiles; t += kWaves) {
    const int trow = t / tiles_c, tcol = t - trow * tiles_c;
    const int row = 8 * trow + (lane >> 3), col = 8 * tcol + (lane & 7);
    const bool in = row < rows && col < cols;
    bool is_known = false;
    if (in) {
      const int v = row * cols + col;
      const P2 pt = kmap::cell_centre(cfg, row, col);
      int st = 0;  // LOGODDS_UNKNOWN
      for (int n = lmc[v]; n > 0; --n) st = fsm.landmark(st);
      for (int i = 0; i < P; ++i) {  // (k_og_cost's walk, up to pose index P)
        if (use_bbox && (row < c.bbox[4 * i] || row > c.bbox[4 * i + 1] || col < c.bbox[4 * i + 2] || col > c.bbox[4 * i + 3])) continue;
        const Pose ps{c.sp[4 * i], c.sp[4 * i + 1], c.sp[4 * i + 2], c.sp[4 * i + 3]};
        const double gx = ps.x - pt.x, gy = ps.y - pt.y;
        if (!(gx * gx + gy * gy < S.r2_max_lt)) continue;
        if (!kmap::in_fov(S, ps, pt)) continue;
        const int nst = fsm.seen(st);
        if (nst == st) break;
        st = nst;
      }
      plane[v] = (uint8_t)st;
      is_known = live[v] < cfg.occupancy_threshold;
    }
    n_known += __popcll(__ballot(is_known));
  }
  if (lane == 0) kred[wave] = n_known;
  __syncthreads();
  if (tid == 0) {
    int k = 0;
    for (int w = 0; w < kWaves; ++w) k += kred[w];
    known[env] = k;
  }
}

// One workgroup per leaf: candidates in k_og_cost's layout, base / known as k_og_tree_base left them for the leaf's environment;
// ent_out / cost_out [gridDim.x], dist_out [gridDim.x][2], any of them null - what k_og_cost writes there, bit for bit.
__global__ __launch_bounds__(kT) void k_og_tree_cost(DRLGX_KS_PARAM, const int32_t *cand_env, const double *actions,
                                                     const int32_t *n_actions, const uint8_t *base, const int32_t *known, double *ent_out,
                                                     double *cost_out, double *dist_out) {
  const DrlgxState &S = DRLGX_KS_REF;
  extern __shared__ __attribute__((aligned(16))) double og_smem[];
  const drlgx_config &cfg = S.cfg;
  const int tid = drlgx_tid(), lane = tid & 63, wave = tid >> 6, ci = blockIdx.x;
  const int env = cand_env[ci];
  const int K = n_actions[ci];
  const bool env_ok = env >= 0 && env < S.n_envs;
  const int P = env_ok ? S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_P] : 0;
  const int V = S.V;
  if (!env_ok || K < 0 || K > S.A_max || P < 1 || P > S.P_max) {  // (the tree's kernel refused such a call: flag it, touch nothing)
    if (tid == 0) atomicMin(S.status, DRLGX_E_CAPACITY);
    return;
  }
  kmap::MapCtx c;  // (the leaf's K new poses only)
  c.sp = og_smem;
  double *red = c.sp + (size_t)S.A_max * 4, *sdist = red + kWaves, *hs = sdist + 1;
  c.bbox = reinterpret_cast<int *>(hs + DRLGX_LO_TAB);
  c.P = K;
  const double *ep = S.est_pose + (size_t)env * S.P_max * 4;
  const double *act = actions + (size_t)ci * S.A_max * 3;

  // ---- staging: one lane per new pose (the first lanes); the plan's distance and the entropy table on the last ones ----
  for (int b = tid; b < K; b += kT) {
    const Pose ps = kem::leaf_pose(ep, P, act, P + b);
    c.sp[4 * b] = ps.x; c.sp[4 * b + 1] = ps.y; c.sp[4 * b + 2] = ps.c; c.sp[4 * b + 3] = ps.s;
    kmap::bbox_origin(S, c.bbox + 4 * b, ps.x, ps.y);
  }
  if (tid == kT - 1) *sdist = kem::plan_distance(cfg, act, K);
  const int hst = kT - 2 - tid;  // (lo_ntab <= DRLGX_LO_TAB < kT - 1)
  if (hst >= 0 && hst < S.lo_ntab) {
    const double pv = S.lo_pv[hst];
    hs[hst] = -pv * log(pv) - (1.0 - pv) * log(1.0 - pv);
  }
  __syncthreads();
  const bool use_bbox = !S.bbox_noop;
  if (use_bbox) kmap::bbox_sweep(S, c);

  // ---- cell pass: k_og_cost's tiles on k_og_cost's waves and lanes ----
  const int cols = S.cols, rows = S.rows;
  const int tiles_c = (cols + 7) >> 3, ntiles = ((rows + 7) >> 3) * tiles_c;
  const kmap::LadderFsm fsm{S.lo_tocc, S.lo_tfree, S.lo_tflag};
  const uint8_t *plane = base + (size_t)env * S.Vu;
  double s_h = 0.0;
  for (int t = wave; t < ntiles; t += kWaves) {
    const int trow = t / tiles_c, tcol = t - trow * tiles_c;
    const int row = 8 * trow + (lane >> 3), col = 8 * tcol + (lane & 7);
    if (!(row < rows && col < cols)) continue;
    const P2 pt = kmap::cell_centre(cfg, row, col);
    int st = plane[row * cols + col];
    for (int i = 0; i < K; ++i) {
      if (use_bbox && (row < c.bbox[4 * i] || row > c.bbox[4 * i + 1] || col < c.bbox[4 * i + 2] || col > c.bbox[4 * i + 3])) continue;
      const Pose ps{c.sp[4 * i], c.sp[4 * i + 1], c.sp[4 * i + 2], c.sp[4 * i + 3]};
      const double gx = ps.x - pt.x, gy = ps.y - pt.y;
      if (!(gx * gx + gy * gy < S.r2_max_lt)) continue;
      if (!kmap::in_fov(S, ps, pt)) continue;
      const int nst = fsm.seen(st);
      if (nst == st) break;
      st = nst;
    }
    s_h += hs[st];
  }
  s_h = kmap::wave_sum63(s_h);
  if (lane == 63) red[wave] = s_h;
  __syncthreads();
  if (tid == 0) {
    double h = 0.0;
    for (int w = 0; w < kWaves; ++w) h += red[w];
    if (ent_out) ent_out[ci] = h;
    if (cost_out || dist_out) {
      const double pk = (double)known[env] / (double)V;
      const double dw = cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * pk;
      if (cost_out) cost_out[ci] = h + *sdist * dw;
      if (dist_out) {
        dist_out[2 * ci] = *sdist;
        dist_out[2 * ci + 1] = dw;
      }
    }
  }
}

// ---- the SLAM-OG-Shannon cost (calculateUncertainty_SLAM_OG_SHANNON, Planner2D.cpp:394-416): the entropy above weighed against the
// landmarks' uncertainty.  sqrt(det) of a landmark's 2x2 covariance given as (xx, xy, yy):
__device__ inline double sqrt_det2(double xx, double xy, double yy) { return sqrt(xx * yy - xy * xy); }

// The root's two weights (EMPlanner2D::initialize, Planner2D.cpp:1341-1354), one workgroup per environment, from the LIVE belief:
//   w2 = (1 - alpha) / sum_v -p_v ln p_v - (1 - p_v) ln(1 - p_v)     (the live virtual map's probabilities)
//   w1 = alpha / sum_l sqrt(det(inverse(information_l)))             (the live landmark marginals, in slot order)
// Both sums: a thread strides its terms, then the waves' sums in wave order.  The divisions are plain IEEE (no landmark: w1 = inf).
// weights [n_envs][2] = w1, w2.
__global__ __launch_bounds__(kT) void k_slam_og_weights(DRLGX_KS_PARAM, double alpha, double *weights) {
  const DrlgxState &S = DRLGX_KS_REF;
  __shared__ double red[2 * kWaves];
  const int tid = drlgx_tid(), lane = tid & 63, wave = tid >> 6, env = blockIdx.x;
  const int L = S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_L], V = S.V;
  const double *live = S.vm_prob + (size_t)env * V;
  const double *li = S.lm_info + (size_t)env * S.L_max * 3;
  double s_h = 0.0, s_l = 0.0;
  for (int v = tid; v < V; v += kT) {
    const double pv = live[v];
    s_h += -pv * log(pv) - (1.0 - pv) * log(1.0 - pv);
  }
  for (int j = tid; j < L; j += kT) {
    const double a = li[3 * j], b = li[3 * j + 1], d = li[3 * j + 2], det = a * d - b * b;
    s_l += sqrt_det2(d / det, -b / det, a / det);  // covariance() = inverse(information)
  }
  s_h = kmap::wave_sum63(s_h);
  s_l = kmap::wave_sum63(s_l);
  if (lane == 63) {
    red[wave] = s_h;
    red[kWaves + wave] = s_l;
  }
  __syncthreads();
  if (tid == 0) {
    double h = 0.0, sl = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      h += red[w];
      sl += red[kWaves + w];
    }
    weights[2 * env] = alpha / sl;
    weights[2 * env + 1] = (1.0 - alpha) / h;
  }
}

// The blend (Planner2D.cpp:407-413, :418-420), one wave per candidate:
//   slam_uncertainty = sum_l sqrt(det Sigma'(l, l))   over the L slots of the candidate's environment: lane q takes slots q, q + 64, ...
//     in rising order, then the wave's sum - a fixed order, the same candidate gives the same bits;
//   uncertainty = w2 H_leaf + w1 slam_uncertainty;   cost = uncertainty + distance * distance_weight.
// lm_cov [nc][lm_stride][3]: what k_fm2_update left; h_leaf [nc], dist [nc][2]: what k_og_cost left; distance [nc] or null: the
// caller's distance instead of the plan's own; weights [n_envs][2].  unc_out / cost_out [nc], terms_out [nc][2] (H_leaf,
// slam_uncertainty): any of them null.  All arrays start at the launch's first candidate.
__global__ __launch_bounds__(64) void k_slam_og_blend(DRLGX_KS_PARAM, const int32_t *cand_env, const double *lm_cov, int lm_stride,
                                                      const double *h_leaf, const double *dist, const double *distance,
                                                      const double *weights, double *unc_out, double *cost_out, double *terms_out) {
  const DrlgxState &S = DRLGX_KS_REF;
  const int lane = drlgx_tid(), ci = blockIdx.x, env = cand_env[ci];
  const int L = S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_L];
  const double *lc = lm_cov + (size_t)ci * lm_stride * 3;
  double s = 0.0;
  for (int l = lane; l < L; l += 64) s += sqrt_det2(lc[3 * l], lc[3 * l + 1], lc[3 * l + 2]);
  s = kmap::wave_sum63(s);
  if (lane == 63) {
    const double h = h_leaf[ci], unc = weights[2 * env + 1] * h + weights[2 * env] * s;
    if (unc_out) unc_out[ci] = unc;
    if (cost_out) cost_out[ci] = unc + (distance ? distance[ci] : dist[2 * ci]) * dist[2 * ci + 1];
    if (terms_out) {
      terms_out[2 * ci] = h;
      terms_out[2 * ci + 1] = s;
    }
  }
}

}  // namespace kog

size_t drlgx_og_lds_bytes(const DrlgxState &S) { return kog::lds_bytes(S.P_max + S.A_max, S.V); }

void drlgx_launch_og_check(const DrlgxState &S, hipStream_t st, int n_cand, const int32_t *cand_env, const int32_t *n_actions, int *flag) {
  hipLaunchKernelGGL(kog::k_og_check, dim3((n_cand + 63) / 64), dim3(64), 0, st, DRLGX_KS_ARG(S), n_cand, cand_env, n_actions, flag);
}

void drlgx_launch_og_cost(const DrlgxState &S, hipStream_t st, int nc, const int32_t *cand_env, const double *actions,
                          const int32_t *n_actions, double *ent_out, double *cost_out, double *prob_out, double *dist_out) {
  static bool attr_set[32] = {false};
  const void *fns[] = {reinterpret_cast<const void *>(&kog::k_og_cost)};
  drlgx_ensure_lds_attr(attr_set, fns, 1, (int)kmap::kLdsBudget);
  hipLaunchKernelGGL(kog::k_og_cost, dim3(nc), dim3(kog::kT), drlgx_og_lds_bytes(S), st, DRLGX_KS_ARG(S), cand_env, actions, n_actions,
                     ent_out, cost_out, prob_out, dist_out);
}

void drlgx_launch_og_tree_cost(const DrlgxState &S, hipStream_t st, int n_sel, const int32_t *env_sel, int nc, const int32_t *cand_env,
                               const double *actions, const int32_t *n_actions, uint8_t *base, int32_t *known, double *ent_out,
                               double *cost_out, double *dist_out) {
  static bool attr_set[32] = {false};
  const void *fns[] = {reinterpret_cast<const void *>(&kog::k_og_tree_base), reinterpret_cast<const void *>(&kog::k_og_tree_cost)};
  drlgx_ensure_lds_attr(attr_set, fns, 2, (int)kmap::kLdsBudget);
  hipLaunchKernelGGL(kog::k_og_tree_base, dim3(n_sel), dim3(kog::kT), kog::tree_base_lds_bytes(S.P_max, S.V), st, DRLGX_KS_ARG(S), env_sel,
                     base, known);
  hipLaunchKernelGGL(kog::k_og_tree_cost, dim3(nc), dim3(kog::kT), kog::tree_leaf_lds_bytes(S.A_max), st, DRLGX_KS_ARG(S), cand_env, actions,
                     n_actions, base, known, ent_out, cost_out, dist_out);
}

void drlgx_launch_slam_og_weights(const DrlgxState &S, hipStream_t st, double alpha, double *weights) {
  hipLaunchKernelGGL(kog::k_slam_og_weights, dim3(S.n_envs), dim3(kog::kT), 0, st, DRLGX_KS_ARG(S), alpha, weights);
}

void drlgx_launch_slam_og_blend(const DrlgxState &S, hipStream_t st, int nc, const int32_t *cand_env, const double *lm_cov, int lm_stride,
                                const double *h_leaf, const double *dist, const double *distance, const double *weights, double *unc_out,
                                double *cost_out, double *terms_out) {
  hipLaunchKernelGGL(kog::k_slam_og_blend, dim3(nc), dim3(64), 0, st, DRLGX_KS_ARG(S), cand_env, lm_cov, lm_stride, h_leaf, dist, distance,
                     weights, unc_out, cost_out, terms_out);
}
