// Expected look-ahead cost of candidate plans: the leaf evaluation of EMPlanner2D::optimize2
// (src/em_exploration/Planner2D.cpp:1095-1104) for action lists the caller supplies -
//   updateTrajectory_EM(node)                              (:472-551; the covariances: k_fm2.hip, read from the engine's scratch)
//   node->virtual_map = copy of the root's; updateInformation(*node->map)   (VirtualMap.cpp:256-316, :213-229, :364-378)
//   node->uncertainty = calculateUncertainty_EM(node)      (:321-341)
//   node->cost = uncertainty + distance * distance_weight_ (:418-420, :1322-1332)
// without simulating, without noise and without re-solving.  The leaf's map holds EVERY pose as a core pose with
// information = Sigma_i^-1 (cov.inverse(), :521-523): the P old ones at the current estimate, one per action at the noise-free
// predicted pose chained from the last estimate.  The leaf's virtual map is a copy of the root's whose information is rebuilt;
// its probabilities stay the live environment's.  Nothing of the live environment is written.  (k_em_cost<true>: the leaves of the
// Dubins control model, whose edges have non-core steps that stay out of the leaf's map - see the kernel.)
//
// One workgroup per candidate.  The P + K poses are staged in LDS once (x y c s, the LLT factor of the information in the layout
// kmap::predict_info reads, the skip flag).  The cell pass is cell-centric: a wave takes an 8 x 8 tile of cells, a lane walks the
// poses in trajectory order for its cell - first hit replaces I / sigma0^2, later hits are fused - with the 2 x 2 information in
// registers.  There is no occupancy ladder and no "sees me" mask here, so the pose-centric pair list of k_map.hip with its LDS
// atomics is not needed.  The three sums are reduced within a wave, then across the waves through LDS in wave order: repeated
// calls give the same bits.  Part of the k_step.hip unity build: kmap's device functions as they are, and -ffp-contract=off
// for the gates.
#include "drlgx_dev.h"

namespace kem {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kSp = 4, kSl = 9;  // doubles per pose: x y c s | LLT factor (. l10 . l20 l21 . r00 r11 r22)

__host__ __device__ inline size_t lds_bytes(int cap) {
  return ((size_t)cap * (kSp + kSl) + 3 * kWaves + 1) * sizeof(double) + (size_t)cap * sizeof(int);
}

// Pose i of a leaf's trajectory: the P old poses at the current estimate (ep), the new ones the noise-free chain from the last
// estimate, as k_fm2_update chains them
__device__ __forceinline__ Pose leaf_pose(const double *ep, int P, const double *act, int i) {
  Pose ps{ep[4 * min(i, P - 1)], ep[4 * min(i, P - 1) + 1], ep[4 * min(i, P - 1) + 2], ep[4 * min(i, P - 1) + 3]};
  for (int b = 0; b <= i - P; ++b) ps = compose(ps, make_pose(act[3 * b], act[3 * b + 1], act[3 * b + 2]));
  return ps;
}

// distance of a plan, accumulated as the look-ahead accumulates it (Planner2D.cpp:1440, ksim: dist += sqrt(x^2 + y^2 +
// angle_weight * theta^2), theta = Pose2::theta())
__device__ __forceinline__ double plan_distance(const drlgx_config &cfg, const double *act, int K) {
  double dist = 0.0;
  for (int b = 0; b < K; ++b) {
    const double ox = act[3 * b], oy = act[3 * b + 1];
    const double th = theta_of(make_pose(ox, oy, act[3 * b + 2]));
    dist = dist + sqrt(ox * ox + oy * oy + cfg.angle_weight * (th * th));
  }
  return dist;
}

// cov: [gridDim.x][cov_stride][9], the covariances k_fm2_update left for the same candidates; cand_env / actions / n_actions and the
// outputs (any of them null) start at this launch's first candidate.
// kSteps: the leaf of a tree whose edges have intermediate steps (the Dubins control model, Planner2D.cpp:472-551): `core`
// ([candidate][max_actions] or null = every action) marks the actions whose pose enters the leaf's map - updateTrajectory_EM adds
// the last pose of every edge only; a non-core step still moves the pose chain -, and `distance` ([candidate] or null) is the
// leaf's distance as the tree accumulated it (:293-303), used instead of plan_distance.  kSteps = false reads neither.
template <bool kSteps>
__global__ __launch_bounds__(kT) void k_em_cost(DRLGX_KS_PARAM, const int32_t *cand_env, const double *actions, const int32_t *n_actions,
                                                const double *cov, int cov_stride, int algorithm, double *unc_out, double *cost_out,
                                                double *info_out, const uint8_t *core, const double *distance) {
  const DrlgxState &S = DRLGX_KS_REF;
  extern __shared__ __attribute__((aligned(16))) double em_smem[];
  const drlgx_config &cfg = S.cfg;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ci = blockIdx.x;
  const int env = cand_env[ci];
  const int P = S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_P], K = n_actions[ci];
  const int cap = S.P_max + S.A_max, np = P + K;
  if (env < 0 || env >= S.n_envs || K < 0 || K > S.A_max || P < 1 || P > S.P_max) {  // (the host checked: flag it, touch nothing)
    if (tid == 0) atomicMin(S.status, DRLGX_E_CAPACITY);
    return;
  }
  double *sp = em_smem, *sl = sp + (size_t)cap * kSp, *red = sl + (size_t)cap * kSl, *sdist = red + 3 * kWaves;
  int *pskip = reinterpret_cast<int *>(sdist + 1);
  const double *ep = S.est_pose + (size_t)env * S.P_max * 4;
  const double *act = actions + (size_t)ci * S.A_max * 3;
  const double *cv = cov + (size_t)ci * cov_stride * 9;

  // ---- pose staging: one lane per pose ----
  for (int i = tid; i < np; i += kT) {
    const Pose ps = leaf_pose(ep, P, act, i);
    sp[4 * i] = ps.x; sp[4 * i + 1] = ps.y; sp[4 * i + 2] = ps.c; sp[4 * i + 3] = ps.s;
    if (kSteps && core && i >= P && !core[(size_t)ci * S.A_max + (i - P)]) {  // not in the leaf's map: nothing of it is factored
      pskip[i] = 1;
      continue;
    }
    // information = cov.inverse() (Planner2D.cpp:521-523): cofactors of the symmetric 3 x 3
    const double *c = cv + (size_t)i * 9;
    const double c00 = c[0], c10 = c[3], c20 = c[6], c11 = c[4], c21 = c[7], c22 = c[8];
    const double k00 = c11 * c22 - c21 * c21, k10 = c20 * c21 - c10 * c22, k20 = c10 * c21 - c20 * c11;
    const double id = 1.0 / (c00 * k00 + c10 * k10 + c20 * k20);
    const double i00 = k00 * id, i10 = k10 * id, i20 = k20 * id;
    const double i11 = (c00 * c22 - c20 * c20) * id, i21 = (c10 * c20 - c00 * c21) * id, i22 = (c00 * c11 - c10 * c10) * id;
    int skip = det3s(i00, i10, i20, i11, i21, i22) < 1e-10 ? 1 : 0;  // VirtualMap.cpp:293-294
    // state.information.llt(), factored once per pose as kmap::pose_setup factors it.  Sigma_i is SPD: a pivot that is not a
    // positive finite number is a bad solve - the pose is left out and the status word says so
    double *o = sl + 9 * i;
    const double d0 = i00;
    const double r00 = rsqrt_n1(d0);
    const double l10 = i10 * r00, l20 = i20 * r00;
    const double d1 = i11 - l10 * l10;
    const double r11 = rsqrt_n1(d1);
    const double l21 = (i21 - l20 * l10) * r11;
    const double d2 = i22 - l20 * l20 - l21 * l21;
    const double r22 = rsqrt_n1(d2);
    const double kInf = __builtin_huge_val();
    if (!skip && !(d0 > 0.0 && d0 < kInf && d1 > 0.0 && d1 < kInf && d2 > 0.0 && d2 < kInf)) {
      skip = 1;
      atomicMin(S.status, DRLGX_E_NUMERIC);
    }
    o[1] = l10; o[3] = l20; o[4] = l21;
    o[6] = r00; o[7] = r11; o[8] = r22;
    pskip[i] = skip;
  }
  if (tid == kT - 1) *sdist = kSteps && distance ? distance[ci] : plan_distance(cfg, act, K);
  __syncthreads();

  // ---- cell pass: one 8 x 8 tile of cells per wave and round (lane = 8 (row mod 8) + (col mod 8), as kmap::cell_pass) ----
  const int cols = S.cols, rows = S.rows;
  const int tiles_c = (cols + 7) >> 3, ntiles = ((rows + 7) >> 3) * tiles_c;
  const double i0 = S.vm_i0;
  const double *prob = S.vm_prob + (size_t)env * S.V;
  double *iout = info_out ? info_out + (size_t)ci * S.V * 3 : nullptr;
  double s_tr = 0.0, s_det = 0.0, s_known = 0.0;
  for (int t = wave; t < ntiles; t += kWaves) {
    const int trow = t / tiles_c, tcol = t - trow * tiles_c;
    const int row = 8 * trow + (lane >> 3), col = 8 * tcol + (lane & 7);
    if (!(row < rows && col < cols)) continue;
    const int v = row * cols + col;
    const double pv = prob[v];
    const P2 pt = kmap::cell_centre(cfg, row, col);
    double axx = i0, axy = 0.0, ayy = i0;
    bool u = false;
    for (int i = 0; i < np; ++i) {
      if (pskip[i]) continue;
      const Pose ps{sp[4 * i], sp[4 * i + 1], sp[4 * i + 2], sp[4 * i + 3]};
      // (the window of a pose: only cells within max_range can pass predict_cell's own range gate)
      const double gx = pt.x - ps.x, gy = pt.y - ps.y;
      if (!(gx * gx + gy * gy < S.r2_max_lt)) continue;
      double bxx, bxy, byy;
      if (!kmap::predict_cell<true>(S, ps, sl + 9 * i, pt, bxx, bxy, byy)) continue;
      if (!u) {  // the first update of an untouched cell replaces the prior (VirtualMap.cpp:307-313)
        axx = bxx; axy = bxy; ayy = byy;
        u = true;
      } else {
        kmap::ci_fuse(axx, axy, ayy, bxx, bxy, byy);
      }
    }
    if (iout) {
      iout[3 * (size_t)v] = axx; iout[3 * (size_t)v + 1] = axy; iout[3 * (size_t)v + 2] = ayy;
    }
    // calculateUncertainty_EM (Planner2D.cpp:321-341): trace and determinant of the covariance (= information^-1, 2 x 2)
    const double rdet = rcp_n1(axx * ayy - axy * axy);
    const double tr = (axx + ayy) * rdet;
    const double wgt = pv > 0.49 ? 1.0 : 0.0;
    s_tr += wgt * tr;
    s_det += wgt * rdet;
    if (pv < cfg.occupancy_threshold) s_known += 1.0;  // (Planner2D.cpp:1322-1325)
  }

  // ---- reductions: within a wave, then across the waves in wave order ----
  s_tr = kmap::wave_sum63(s_tr);
  s_det = kmap::wave_sum63(s_det);
  s_known = kmap::wave_sum63(s_known);
  if (lane == 63) {
    red[wave] = s_tr;
    red[kWaves + wave] = s_det;
    red[2 * kWaves + wave] = s_known;
  }
  __syncthreads();
  if (tid == 0) {
    double r3[3];
    for (int k = 0; k < 3; ++k) {
      r3[k] = 0.0;
      for (int w = 0; w < kWaves; ++w) r3[k] += red[k * kWaves + w];
    }
    const double unc = algorithm == DRLGX_ALG_EM_DOPT ? r3[1] : r3[0];
    if (unc_out) unc_out[ci] = unc;
    if (cost_out) {
      const double pk = r3[2] / (double)S.V;
      const double dw = cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * pk;
      cost_out[ci] = unc + *sdist * dw;
    }
  }
}

}  // namespace kem

size_t drlgx_em_lds_bytes(const DrlgxState &S) { return kem::lds_bytes(S.P_max + S.A_max); }

void drlgx_launch_em_cost(const DrlgxState &S, hipStream_t st, int nc, const int32_t *cand_env, const double *actions,
                          const int32_t *n_actions, const uint8_t *core, const double *distance, const double *cov, int cov_stride,
                          int algorithm, double *unc_out, double *cost_out, double *info_out) {
  static bool attr_set[32] = {false};
  const void *fns[] = {reinterpret_cast<const void *>(&kem::k_em_cost<false>), reinterpret_cast<const void *>(&kem::k_em_cost<true>)};
  drlgx_ensure_lds_attr(attr_set, fns, 2, (int)kmap::kLdsBudget);
  if (core || distance)
    hipLaunchKernelGGL(kem::k_em_cost<true>, dim3(nc), dim3(kem::kT), drlgx_em_lds_bytes(S), st, DRLGX_KS_ARG(S), cand_env, actions,
                       n_actions, cov, cov_stride, algorithm, unc_out, cost_out, info_out, core, distance);
  else
    hipLaunchKernelGGL(kem::k_em_cost<false>, dim3(nc), dim3(kem::kT), drlgx_em_lds_bytes(S), st, DRLGX_KS_ARG(S), cand_env, actions,
                       n_actions, cov, cov_stride, algorithm, unc_out, cost_out, info_out, core, distance);
}
