// What the SLAM stages of the unity build k_step.hip share besides the sweep primitives (k_sweep.hip): the capacity
// constants, the per-factor record and its linearisation (linearize_br), the pose-side factor blocks (pose_block for the
// pose-chain solver k_slam_arrow.hip; prior_factor / odo_factor / own_factor_add, the same sums in pieces, for the dense
// solver k_slam.hip), and what the fused step kernel hands a SLAM stage that runs beside its simulator wave (SubBarrier,
// SimBox: k_slam.hip, k_inc.hip).
#pragma once
#include "k_sweep.hip"
#include "arrow_carve.h"
#include "slam_carve.h"
namespace kslam {
#pragma clang fp contract(fast)
// ---- capacities of the SLAM kernels (one 512-thread workgroup per instance, the whole dynamic LDS) ----
constexpr int kLdsBudget = 160 * 1024;
// (the dense solver's capacities kFastTiles and kDenseTiles: slam_carve.h, with its layout)
// (the pose-chain solver's capacities kFastTilesArrow and kArrowRegTiles: arrow_carve.h, with its layout)
static_assert(kFastTilesArrow == 8, "inc_plan (k_inc.hip) spells the reach of k_step_arrow out as 16 * 8");

constexpr int REC = 12;  // per-factor record: [0..5] Jx (2x3) -> later G (3x2); [6..9] Jl (2x2) -> later partial; [10..11] e
// (12 doubles put the 64-bit accesses of a half-wave that walks consecutive records on 8 banks; a stride of 13 is
// conflict-free and measured SLOWER - G 1.3 -> 2.3 us, Schur 7.8 -> 9.0, landmark marginals 4.4 -> 6.4: the records lose
// their 16-byte alignment and with it the 128-bit loads)

// (linearize_br is shared with the incremental update (k_inc.hip), whose fused and staged forms must round alike although they
// are inlined into differently shaped code: contraction decided in the front end for it)
#pragma clang fp contract(on)
// BearingRangeFactor linearised at (pose, landmark) (SLAM2D.cpp:91-124; gtsam BearingRangeFactor).  d = the landmark in the
// pose frame, n = |d|, (c, s) = d / n: the predicted bearing is atan2(s, c) and never needed as an angle - the error
// Rot2 Local(measured, predicted) is taken from (c, s) directly - and the predicted range is n; the range Jacobians are
// (-c, -s, 0) for the pose and R (c, s) for the landmark.  One square root, one division, one sincos, one atan2 (the
// composition of bearing_of / range_of - two atan2, four trigonometric calls, two roots, six divisions - took most of the
// 2.9 us the factor tables cost).
__device__ __forceinline__ void linearize_br(const double *tp, const double *tl, double bm, double rm, double *rec) {
  Pose ps{tp[0], tp[1], tp[2], tp[3]};
  P2 lm{tl[0], tl[1]};
  const P2 d = transform_to(ps, lm);
  const double d2 = d.x * d.x + d.y * d.y, n = sqrt(d2);
  double sm, cm;
  sincos(bm, &sm, &cm);
  if (n > 1e-5) {
    const double in = 1.0 / n;
    const double c = d.x * in, s = d.y * in;
    const double a = -s * in, b = c * in;  // -d.y / d2, d.x / d2
    rec[0] = -a;
    rec[1] = -b;
    rec[2] = a * d.y - b * d.x;
    rec[3] = -c;
    rec[4] = -s;
    rec[5] = 0.0;
    rec[6] = a * ps.c - b * ps.s;
    rec[7] = a * ps.s + b * ps.c;
    rec[8] = ps.c * c - ps.s * s;
    rec[9] = ps.s * c + ps.c * s;
    rec[10] = atan2(-sm * c + cm * s, cm * c + sm * s);
    rec[11] = n - rm;
  } else {  // (a landmark on top of the pose: the conventions of bearing_of / range_of)
    double Jx[6], Jl[4];
    (void)bearing_of<true>(ps, lm, Jx, Jl);
    const double rp = range_of<true>(ps, lm, Jx + 3, Jl + 2);
    for (int k = 0; k < 6; ++k) rec[k] = Jx[k];
    for (int k = 0; k < 4; ++k) rec[6 + k] = Jl[k];
    rec[10] = atan2(-sm, cm);
    rec[11] = rp - rm;
  }
}

__device__ __forceinline__ size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }

#pragma clang fp contract(fast)
// iterate the poses p (ascending) whose bit is set in the W-word mask at `mk`
#define FOR_EACH_OBSERVING_POSE(mk, W, p)                                      \
  for (int _w = 0; _w < (W); ++_w)                                            \
    for (unsigned long long _m = (mk)[_w]; _m; _m &= _m - 1)                  \
      if (const int p = 64 * _w + __ffsll((long long)_m) - 1; true)

// Pose i's diagonal block B (3x3, full) and gradient g of the prior / odometry (odo[i] = measured odometry between the
// poses i and i + 1: x, y, cos, sin) / own bearing-range factors linearised at thp, and - for i + 1 < P - the block O = (i + 1, i) of the odometry factor i (SLAM2D.cpp:44-89; records: linearize_br)
__device__ __forceinline__ void pose_block(const DrlgxState &S, int inst, const double *thp, const double *odo, const double *rec, const int *mstart,
                                           int i, int P, double wb, double wr, double *B, double *g, double *O) {
  const drlgx_config &cfg = S.cfg;
  for (int k = 0; k < 9; ++k) B[k] = 0.0;
  for (int k = 0; k < 3; ++k) g[k] = 0.0;
  const Pose ti{thp[4 * i], thp[4 * i + 1], thp[4 * i + 2], thp[4 * i + 3]};
  if (i == 0) {  // prior (SLAM2D.cpp:44-57): e = Local(prior, x0), J = diag(R_h^T, 1), W = information
    const double *pr = S.prior + (size_t)inst * DRLGX_PRIOR_STRIDE;
    const Pose h = between(Pose{pr[0], pr[1], pr[2], pr[3]}, ti, nullptr);
    const double e[3] = {h.x, h.y, theta_of(h)};
    const double J[9] = {h.c, h.s, 0, -h.s, h.c, 0, 0, 0, 1};
    const double *W = pr + 4;
    double WJ[9], We[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) WJ[r * 3 + c] = W[r * 3] * J[c] + W[r * 3 + 1] * J[3 + c] + W[r * 3 + 2] * J[6 + c];
      We[r] = W[r * 3] * e[0] + W[r * 3 + 1] * e[1] + W[r * 3 + 2] * e[2];
    }
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) B[r * 3 + c] += J[r] * WJ[c] + J[3 + r] * WJ[3 + c] + J[6 + r] * WJ[6 + c];
      g[r] += J[r] * We[0] + J[3 + r] * We[1] + J[6 + r] * We[2];
    }
  }
  const double wo[3] = {1.0 / (cfg.translation_noise * cfg.translation_noise),
                        1.0 / (cfg.translation_noise * cfg.translation_noise),
                        1.0 / (cfg.rotation_noise * cfg.rotation_noise)};
  if (i > 0) {  // odometry factor i-1 seen from its second key: J2 = Hlocal (SLAM2D.cpp:59-89)
    const double *oo = odo + 4 * (i - 1);
    const Pose tm{thp[4 * (i - 1)], thp[4 * (i - 1) + 1], thp[4 * (i - 1) + 2], thp[4 * (i - 1) + 3]};
    const Pose hx = between(tm, ti, nullptr);
    const Pose h = between(Pose{oo[0], oo[1], oo[2], oo[3]}, hx, nullptr);
    const double e[3] = {h.x, h.y, theta_of(h)};
    const double J2[9] = {h.c, h.s, 0, -h.s, h.c, 0, 0, 0, 1};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        B[r * 3 + c] += J2[r] * wo[0] * J2[c] + J2[3 + r] * wo[1] * J2[3 + c] + J2[6 + r] * wo[2] * J2[6 + c];
      g[r] += J2[r] * wo[0] * e[0] + J2[3 + r] * wo[1] * e[1] + J2[6 + r] * wo[2] * e[2];
    }
  }
  if (i + 1 < P) {  // odometry factor i from its first key: J1 = Hlocal * H1; also block (i+1, i) = J2^T W J1
    const double *oo = odo + 4 * i;
    const Pose tn{thp[4 * (i + 1)], thp[4 * (i + 1) + 1], thp[4 * (i + 1) + 2], thp[4 * (i + 1) + 3]};
    double H1[9];
    const Pose hx = between(ti, tn, H1);
    const Pose h = between(Pose{oo[0], oo[1], oo[2], oo[3]}, hx, nullptr);
    const double e[3] = {h.x, h.y, theta_of(h)};
    const double Hl[9] = {h.c, h.s, 0, -h.s, h.c, 0, 0, 0, 1};
    double J1[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) J1[r * 3 + c] = Hl[r * 3] * H1[c] + Hl[r * 3 + 1] * H1[3 + c] + Hl[r * 3 + 2] * H1[6 + c];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        B[r * 3 + c] += J1[r] * wo[0] * J1[c] + J1[3 + r] * wo[1] * J1[3 + c] + J1[6 + r] * wo[2] * J1[6 + c];
      g[r] += J1[r] * wo[0] * e[0] + J1[3 + r] * wo[1] * e[1] + J1[6 + r] * wo[2] * e[2];
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        O[r * 3 + c] = Hl[r] * wo[0] * J1[c] + Hl[3 + r] * wo[1] * J1[3 + c] + Hl[6 + r] * wo[2] * J1[6 + c];
  }
  for (int m = mstart[i]; m < mstart[i + 1]; ++m) {  // own bearing-range factors
    const double *l = rec + (size_t)REC * m;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) B[r * 3 + c] += l[r] * wb * l[c] + l[3 + r] * wr * l[3 + c];
      g[r] += l[r] * wb * l[10] + l[3 + r] * wr * l[11];
    }
  }
}

// ---- pose_block in pieces, for the LDS-resident solver's front end (one thread per pose ran the whole of it: ~3 us of
// serial fp64 per pose - two atan2 among it - plus ~0.3 us per own factor, in ONE wave, while the others idled) ----
// lower triangle (xx, yx, yy, tx, ty, tt) + gradient of one bearing-range factor seen from its pose, added to B6 / g
__device__ __forceinline__ void own_factor_add(const double *l, double wb, double wr, double *B6, double *g) {
  for (int r = 0, q = 0; r < 3; ++r) {
    for (int c = 0; c <= r; ++c, ++q) B6[q] += l[r] * wb * l[c] + l[3 + r] * wr * l[3 + c];
    g[r] += l[r] * wb * l[10] + l[3 + r] * wr * l[11];
  }
}
// the prior on pose 0 (SLAM2D.cpp:44-57): its block (lower triangle) and gradient
__device__ __forceinline__ void prior_factor(const DrlgxState &S, int inst, const double *thp, double *B6, double *g) {
  const Pose t0{thp[0], thp[1], thp[2], thp[3]};
  const double *pr = S.prior + (size_t)inst * DRLGX_PRIOR_STRIDE;
  const Pose h = between(Pose{pr[0], pr[1], pr[2], pr[3]}, t0, nullptr);
  const double e[3] = {h.x, h.y, theta_of(h)};
  const double J[9] = {h.c, h.s, 0, -h.s, h.c, 0, 0, 0, 1};
  const double *W = pr + 4;
  double WJ[9], We[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) WJ[r * 3 + c] = W[r * 3] * J[c] + W[r * 3 + 1] * J[3 + c] + W[r * 3 + 2] * J[6 + c];
    We[r] = W[r * 3] * e[0] + W[r * 3 + 1] * e[1] + W[r * 3 + 2] * e[2];
  }
  for (int r = 0, q = 0; r < 3; ++r) {
    for (int c = 0; c <= r; ++c, ++q) B6[q] = J[r] * WJ[c] + J[3 + r] * WJ[3 + c] + J[6 + r] * WJ[6 + c];
    g[r] = J[r] * We[0] + J[3 + r] * We[1] + J[6 + r] * We[2];
  }
}
// odometry factor i (poses i, i + 1; SLAM2D.cpp:59-89) linearised ONCE: what it adds to the block / gradient of its first
// key (C1, g1) and of its second key (C2, g2), and the off-diagonal block O = (i + 1, i)
__device__ __forceinline__ void odo_factor(const DrlgxState &S, const double *thp, const double *odo, int i, double *C1, double *g1,
                                           double *C2, double *g2, double *O) {
  const double wt = S.w_trans, wr = S.w_rot;  // W = diag(wt, wt, wr)
  const Pose ti{thp[4 * i], thp[4 * i + 1], thp[4 * i + 2], thp[4 * i + 3]};
  const Pose tn{thp[4 * (i + 1)], thp[4 * (i + 1) + 1], thp[4 * (i + 1) + 2], thp[4 * (i + 1) + 3]};
  const double *oo = odo + 4 * i;
  double H1[9];
  const Pose hx = between(ti, tn, H1);
  const Pose h = between(Pose{oo[0], oo[1], oo[2], oo[3]}, hx, nullptr);
  const double e0 = h.x, e1 = h.y, e2 = theta_of(h);
  // Jacobians: second key Hl = [h.c h.s 0; -h.s h.c 0; 0 0 1], first key J1 = Hl H1 with H1 = [. . .; . . .; 0 0 -1] - the
  // zero / unit entries are written out (the generic 3x3 products spend two thirds of their operations on them)
  const double j00 = h.c * H1[0] + h.s * H1[3], j01 = h.c * H1[1] + h.s * H1[4], j02 = h.c * H1[2] + h.s * H1[5];
  const double j10 = h.c * H1[3] - h.s * H1[0], j11 = h.c * H1[4] - h.s * H1[1], j12 = h.c * H1[5] - h.s * H1[2];
  // C1 = J1^T W J1 (lower: xx yx yy tx ty tt), g1 = J1^T W e;  row 2 of J1 = (0, 0, -1)
  C1[0] = wt * (j00 * j00 + j10 * j10);
  C1[1] = wt * (j01 * j00 + j11 * j10);
  C1[2] = wt * (j01 * j01 + j11 * j11);
  C1[3] = wt * (j02 * j00 + j12 * j10);
  C1[4] = wt * (j02 * j01 + j12 * j11);
  C1[5] = wt * (j02 * j02 + j12 * j12) + wr;
  g1[0] = wt * (j00 * e0 + j10 * e1);
  g1[1] = wt * (j01 * e0 + j11 * e1);
  g1[2] = wt * (j02 * e0 + j12 * e1) - wr * e2;
  // C2 = Hl^T W Hl, g2 = Hl^T W e
  const double n2 = h.c * h.c + h.s * h.s;
  C2[0] = wt * n2; C2[1] = 0.0; C2[2] = wt * n2; C2[3] = 0.0; C2[4] = 0.0; C2[5] = wr;
  g2[0] = wt * (h.c * e0 - h.s * e1);
  g2[1] = wt * (h.s * e0 + h.c * e1);
  g2[2] = wr * e2;
  // O = Hl^T W J1 = block (i + 1, i)
  O[0] = wt * (h.c * j00 - h.s * j10); O[1] = wt * (h.c * j01 - h.s * j11); O[2] = wt * (h.c * j02 - h.s * j12);
  O[3] = wt * (h.s * j00 + h.c * j10); O[4] = wt * (h.s * j01 + h.c * j11); O[5] = wt * (h.s * j02 + h.c * j12);
  O[6] = 0.0; O[7] = 0.0; O[8] = -wr;
}

// ---- software barrier among the waves that run the SLAM front end beside the simulator wave (k_step) ----
// A monotonic LDS counter: every participating wave adds one and waits (lane 0, s_sleep) until all have arrived.  The
// hardware barrier cannot be used there: the simulator wave does not take part.
struct SubBarrier {
  int *cnt;
  int nwaves, phase;
  __device__ __forceinline__ void sync(int lane) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    ++phase;
    if (lane == 0) {
      __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < nwaves * phase) __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
};

// What the simulator wave of k_step appended in this step, left in LDS (ksim::measure): factor M0 + r = (newest pose,
// landmark slot[r], bearing br[2 r], range br[2 r + 1]), new landmark L0 + r at lm[2 r], lm[2 r + 1].  br == null: not there.
struct SimBox {
  const double *br;
  const int *slot;
  const double *lm;
};
#pragma clang fp contract(off)
}  // namespace kslam
