// EKF-style covariance propagate / update without re-solving: FastMarginals2::update / propagate
// (src/em_exploration/FastMarginals.cpp:188-321) fed the way the EM planner feeds it
// (src/em_exploration/Planner2D.cpp:652-737 updateNodeInformation_EM, :472-551 updateTrajectory_EM):
//   * one new pose per action, predicted noise-free from the last pose's ESTIMATE; its odometry factor linearised at
//     (linearisation point of the last pose | predicted pose) gives   cov1 = H1 (H0 cov0 H0^T + I) H1^T,
//     F_b = -H1 H0, Fs_b = F_b Fs_{b-1}   (H0, H1^-1 = the whitened Jacobian blocks);
//   * noise-free bearing-range factors from every new pose to the landmarks of the ESTIMATED map that pass the sensor
//     gates, linearised at (predicted pose | landmark linearisation point): whitened rows A;
//   * Sigma' = Sigma - Sigma A^T (I + A Sigma A^T)^-1 A Sigma on the diagonal block of every pose.
// The joint prior Sigma (FastMarginals::recover) is the dense inverse of the information matrix linearised at the iSAM
// linearisation point: k_fm2_prior builds and inverts it per environment (in HBM, n = 3P + 2L); k_fm2_update then needs
// only blocks of it: T = I + A Sigma A^T is assembled measurement pair by measurement pair from
//   Sigma(l, l'), Sigma(l, x_new b) = Sigma(l, x_last) Fs_b^T, Sigma(x_new a, x_new b) = cov_a F_{a+1}^T ... F_b^T,
// inverted (SPD, Gauss-Jordan), and  Delta_i = -U_i^T T^-1 U_i  with  U_i = A Sigma(., x_i)  (2 rows per measurement).
// k_fm2_update is the sequence of these phases, one function each, with the workgroup's barriers between them:
//   chain (thread 0) | cross: NN | predict: gates, ordered compaction, whitened J | assemble_T | spd_inverse |
//   reduce_block<3> per pose | reduce_block<2> per landmark (kLm)
// Its scratch layout, the measurement cap and the size of the Gauss-Jordan LDS are fm2_carve.h's.
// This is the planner-side primitive of SURVEY.md section 8(f)-1; it is not on the belief-step hot path and is written for
// clarity: one workgroup per environment / candidate, matrices in an HBM scratch, O(n^3) / O(dim^3) sweeps.
#include "drlgx_dev.h"
#include "fm2_carve.h"

namespace kfm2 {

// BearingRangeFactor Jacobians at (pose, point): Jx 2x3 (bearing row, range row), Jl 2x2
__device__ inline void br_jac(const Pose &ps, const P2 &lm, double *Jx, double *Jl) {
  (void)bearing_of<true>(ps, lm, Jx, Jl);
  (void)range_of<true>(ps, lm, Jx + 3, Jl + 2);
}

__device__ inline void mat3_mul(const double *a, const double *b, double *o) {  // o = a b
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3] * b[c] + a[r * 3 + 1] * b[3 + c] + a[r * 3 + 2] * b[6 + c];
}
__device__ inline void mat3_mul_bt(const double *a, const double *b, double *o) {  // o = a b^T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3] * b[c * 3] + a[r * 3 + 1] * b[c * 3 + 1] + a[r * 3 + 2] * b[c * 3 + 2];
}
__device__ inline Pose pose_at(const double *p, int i) { return Pose{p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]}; }

// In-place inverse of a symmetric positive definite n x n matrix (row major, leading dimension ld) by Gauss-Jordan
// sweeps; `col` / `row`: LDS scratch of n doubles each.  Whole workgroup.
__device__ inline void spd_inverse(double *A, int n, int ld, double *col, double *row, int *bad) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int k = 0; k < n; ++k) {
    for (int i = tid; i < n; i += nt) {
      col[i] = A[(size_t)i * ld + k];
      row[i] = A[(size_t)k * ld + i];
    }
    __syncthreads();
    const double p = col[k];
    if (tid == 0 && !(p > 0)) *bad = 1;
    const double ip = 1.0 / p;
    for (size_t e = tid; e < (size_t)n * n; e += nt) {
      const int i = (int)(e / n), j = (int)(e - (size_t)i * n);
      double v;
      if (i == k) v = (j == k) ? ip : row[j] * ip;
      else if (j == k) v = -col[i] * ip;
      else v = A[(size_t)i * ld + j] - col[i] * row[j] * ip;
      A[(size_t)i * ld + j] = v;
    }
    __syncthreads();
  }
}

// The whitened information blocks of the prior factor on pose 0 (ti = its linearisation point), of odometry factor i (poses i,
// i + 1) and of one bearing-range factor.  B12 is the (i, i + 1) block; (i + 1, i) is its transpose.  Bxl is the (pose, landmark)
// block 3x2; (landmark, pose) is its transpose.
__device__ inline void prior_info(const DrlgxState &S, int inst, const Pose &ti, double *B) {  // J = diag(R_h^T, 1), W = the prior information
  const double *pr = S.prior + (size_t)inst * DRLGX_PRIOR_STRIDE;
  const Pose h = between(Pose{pr[0], pr[1], pr[2], pr[3]}, ti, nullptr);
  const double J[9] = {h.c, h.s, 0, -h.s, h.c, 0, 0, 0, 1};
  double WJ[9];
  mat3_mul(pr + 4, J, WJ);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) B[r * 3 + c] = J[r] * WJ[c] + J[3 + r] * WJ[3 + c] + J[6 + r] * WJ[6 + c];
}
__device__ inline void odo_info(const DrlgxState &S, int inst, const double *thp, int i, const double *wo, double *B11, double *B12,
                                double *B22) {
  const double *oo = S.odo + ((size_t)inst * S.P_max + i) * 4;
  double H1[9];
  const Pose hx = between(pose_at(thp, i), pose_at(thp, i + 1), H1);
  const Pose h = between(Pose{oo[0], oo[1], oo[2], oo[3]}, hx, nullptr);
  const double J2[9] = {h.c, h.s, 0, -h.s, h.c, 0, 0, 0, 1};
  double J1[9];
  mat3_mul(J2, H1, J1);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double s11 = 0, s12 = 0, s22 = 0;
      for (int k = 0; k < 3; ++k) {
        s11 += J1[k * 3 + r] * wo[k] * J1[k * 3 + c];
        s12 += J1[k * 3 + r] * wo[k] * J2[k * 3 + c];
        s22 += J2[k * 3 + r] * wo[k] * J2[k * 3 + c];
      }
      B11[r * 3 + c] = s11; B12[r * 3 + c] = s12; B22[r * 3 + c] = s22;
    }
}
__device__ inline void br_info(const Pose &ps, const P2 &lm, double wb, double wr, double *Bxx, double *Bxl, double *Bll) {
  double Jx[6], Jl[4];
  br_jac(ps, lm, Jx, Jl);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Bxx[r * 3 + c] = Jx[r] * wb * Jx[c] + Jx[3 + r] * wr * Jx[3 + c];
    for (int c = 0; c < 2; ++c) Bxl[r * 2 + c] = Jx[r] * wb * Jl[c] + Jx[3 + r] * wr * Jl[2 + c];
  }
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 2; ++c) Bll[r * 2 + c] = Jl[r] * wb * Jl[c] + Jl[2 + r] * wr * Jl[2 + c];
}
// What both prior kernels start from: one environment's counts, its zeroed matrix and the factors' weights
struct PriorCtx {
  int P, L, M, n;
  double *A;                 // sig of this environment, ld = n
  const double *thp, *thl;   // linearisation points
  const int *mp, *ml;        // [M] measurement -> pose, landmark slot
  double wo[3], wb, wr;
};
__device__ inline PriorCtx prior_begin(const DrlgxState &S, int inst, double *sig, size_t sig_stride, int *bad) {
  const int *cnt = S.cnt + (size_t)inst * DRLGX_CNT_STRIDE;
  const drlgx_config &cfg = S.cfg;
  PriorCtx p;
  p.P = cnt[C_P]; p.L = cnt[C_L]; p.M = cnt[C_M]; p.n = 3 * p.P + 2 * p.L;
  p.A = sig + (size_t)inst * sig_stride;
  p.thp = S.th_pose + (size_t)inst * S.P_max * 4;
  p.thl = S.th_lm + (size_t)inst * S.L_max * 2;
  p.mp = S.meas_pose + (size_t)inst * S.M_max;
  p.ml = S.meas_lm + (size_t)inst * S.M_max;
  p.wo[0] = p.wo[1] = 1.0 / (cfg.translation_noise * cfg.translation_noise);
  p.wo[2] = 1.0 / (cfg.rotation_noise * cfg.rotation_noise);
  p.wb = 1.0 / (cfg.bearing_noise * cfg.bearing_noise);
  p.wr = 1.0 / (cfg.range_noise * cfg.range_noise);
  if (threadIdx.x == 0) *bad = 0;
  for (size_t e = threadIdx.x; e < (size_t)p.n * p.n; e += kT) p.A[e] = 0.0;
  __syncthreads();
  return p;
}

// Sigma = (J^T W J)^-1 at the linearisation point of environment blockIdx.x; order: poses (3 each), then landmarks by slot (2 each);
// written to sig + blockIdx.x * sig_stride with leading dimension n = 3P + 2L.  One workgroup per environment.
__global__ __launch_bounds__(kT) void k_fm2_prior(DrlgxState S, double *sig, size_t sig_stride) {
  __shared__ int bad;
  extern __shared__ double lds[];
  const int tid = threadIdx.x, inst = blockIdx.x;
  const PriorCtx p = prior_begin(S, inst, sig, sig_stride, &bad);
  const int P = p.P, n = p.n;
  double *A = p.A;
  // (fp64 atomics: the summation order of a block's contributions is not fixed; this primitive is tolerance-level)
  // m: nr x nc at (r0, c0); both: its transpose at (c0, r0) as well
  auto add = [&](int r0, int c0, int nr, int nc, const double *m, bool both) {
    for (int r = 0; r < nr; ++r)
      for (int c = 0; c < nc; ++c) {
        atomicAdd(&A[(size_t)(r0 + r) * n + c0 + c], m[r * nc + c]);
        if (both) atomicAdd(&A[(size_t)(c0 + c) * n + r0 + r], m[r * nc + c]);
      }
  };
  for (int i = tid; i < P; i += kT) {
    double B11[9], B12[9], B22[9];
    if (i == 0) {
      prior_info(S, inst, pose_at(p.thp, 0), B11);
      add(0, 0, 3, 3, B11, false);
    }
    if (i + 1 < P) {  // odometry factor i: blocks (i,i), (i,i+1), (i+1,i), (i+1,i+1)
      odo_info(S, inst, p.thp, i, p.wo, B11, B12, B22);
      add(3 * i, 3 * i, 3, 3, B11, false);
      add(3 * i, 3 * i + 3, 3, 3, B12, true);
      add(3 * i + 3, 3 * i + 3, 3, 3, B22, false);
    }
  }
  for (int m = tid; m < p.M; m += kT) {
    const int q = p.mp[m], j = p.ml[m];
    double Bxx[9], Bxl[6], Bll[4];
    br_info(pose_at(p.thp, q), P2{p.thl[2 * j], p.thl[2 * j + 1]}, p.wb, p.wr, Bxx, Bxl, Bll);
    add(3 * q, 3 * q, 3, 3, Bxx, false);
    add(3 * q, 3 * P + 2 * j, 3, 2, Bxl, true);
    add(3 * P + 2 * j, 3 * P + 2 * j, 2, 2, Bll, false);
  }
  __syncthreads();
  spd_inverse(A, n, n, lds, lds + n, &bad);
  if (tid == 0 && bad) atomicMin(S.status, DRLGX_E_NUMERIC);
}

// k_fm2_prior with a FIXED summation order, for the caller that promises the same bits from the same belief (drlgx_slam_og_cost):
// no atomics - every block of the information matrix has one owner that adds its contributions in factor order.  Owner of pose i:
// its diagonal block (the prior, odometry factor i - 1, odometry factor i, then its measurements in list order) and the blocks
// (i, i + 1), (i + 1, i).  Owner of landmark j: its diagonal block and every (pose, j), (j, pose) block, measurements in list order.
// One workgroup per environment; sig as k_fm2_prior's.
__global__ __launch_bounds__(kT) void k_fm2_prior_ordered(DrlgxState S, double *sig, size_t sig_stride) {
  __shared__ int bad;
  extern __shared__ double lds[];
  const int tid = threadIdx.x, inst = blockIdx.x;
  const PriorCtx p = prior_begin(S, inst, sig, sig_stride, &bad);
  const int P = p.P, L = p.L, M = p.M, n = p.n;
  double *A = p.A;
  for (int o = tid; o < P + L; o += kT) {
    if (o < P) {
      const int i = o;
      const Pose ti = pose_at(p.thp, i);
      double D[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, B11[9], B12[9], B22[9];
      if (i == 0) {
        prior_info(S, inst, ti, B11);
        for (int q = 0; q < 9; ++q) D[q] += B11[q];
      }
      if (i > 0) {
        odo_info(S, inst, p.thp, i - 1, p.wo, B11, B12, B22);
        for (int q = 0; q < 9; ++q) D[q] += B22[q];
      }
      if (i + 1 < P) {
        odo_info(S, inst, p.thp, i, p.wo, B11, B12, B22);
        for (int q = 0; q < 9; ++q) D[q] += B11[q];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            A[(size_t)(3 * i + r) * n + 3 * i + 3 + c] = B12[r * 3 + c];
            A[(size_t)(3 * i + 3 + c) * n + 3 * i + r] = B12[r * 3 + c];
          }
      }
      for (int m = 0; m < M; ++m) {
        if (p.mp[m] != i) continue;
        const int j = p.ml[m];
        double Bxx[9], Bxl[6], Bll[4];
        br_info(ti, P2{p.thl[2 * j], p.thl[2 * j + 1]}, p.wb, p.wr, Bxx, Bxl, Bll);
        for (int q = 0; q < 9; ++q) D[q] += Bxx[q];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[(size_t)(3 * i + r) * n + 3 * i + c] = D[r * 3 + c];
    } else {
      const int j = o - P, cj = 3 * P + 2 * j;
      const P2 lm{p.thl[2 * j], p.thl[2 * j + 1]};
      double D[4] = {0, 0, 0, 0};
      for (int m = 0; m < M; ++m) {
        if (p.ml[m] != j) continue;
        const int q = p.mp[m];
        double Bxx[9], Bxl[6], Bll[4];
        br_info(pose_at(p.thp, q), lm, p.wb, p.wr, Bxx, Bxl, Bll);
        for (int k = 0; k < 4; ++k) D[k] += Bll[k];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 2; ++c) {  // (only this thread touches column / row block j: plain read-modify-write)
            A[(size_t)(3 * q + r) * n + cj + c] += Bxl[r * 2 + c];
            A[(size_t)(cj + c) * n + 3 * q + r] += Bxl[r * 2 + c];
          }
      }
      for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c) A[(size_t)(cj + r) * n + cj + c] = D[r * 2 + c];
    }
  }
  __syncthreads();
  spd_inverse(A, n, n, lds, lds + n, &bad);
  if (tid == 0 && bad) atomicMin(S.status, DRLGX_E_NUMERIC);
}

// ---- what k_fm2_update and k_fm2_check share: one copy, so that the check counts exactly the measurements the update predicts
// the sensor gates of a predicted measurement (Planner2D.cpp:717-731): pose ps, landmark estimate lm
__device__ __forceinline__ bool in_gate(const drlgx_config &cfg, const Pose &ps, const P2 &lm) {
  const double dx = lm.x - ps.x, dy = lm.y - ps.y, rng = sqrt(dx * dx + dy * dy);
  const double bearing = bearing_of<false>(ps, lm, nullptr, nullptr);
  return rng < cfg.max_range && rng > cfg.min_range && bearing < cfg.max_bearing && bearing > cfg.min_bearing;
}
// one step of the noise-free pose chain: action a = (x y theta) applied to `origin`; *odom = the action as a pose
__device__ __forceinline__ Pose chain_step(const Pose &origin, const double *a, Pose *odom) {
  *odom = make_pose(a[0], a[1], a[2]);
  return compose(origin, *odom);
}

// One candidate of k_fm2_update: its counts, its environment's prior and belief, its scratch (fm2_carve.h)
struct Fm2Ctx {
  int P, L, K, nm;            // old poses, landmarks, new poses, measurements (nm: once `predict` is through)
  const double *Sig;          // prior covariance of the candidate's environment, ld = n
  int n;
  double *cov_new, *F, *Fs;   // [K][9] each
  double *NN;                 // [K][K][9]: Sigma(new a, new b), a <= b
  int *mk, *mj;               // [nm] measurement -> new pose index, landmark slot
  double *J;                  // [nm][10]: whitened Jx (2x3), Jl (2x2)
  double *T;                  // [2 nm][2 nm]
  double *U;                  // this wave's slab
  double *newp;               // [K][4] predicted poses
  const double *thp, *thl;    // linearisation points of the environment's poses / landmarks
  const double *ep, *el;      // their estimates
};
// Sigma(new pose a, new pose b), any order (3x3)
__device__ inline void cov_nn(const Fm2Ctx &c, int a, int b, double *o) {
  if (a <= b) {
    for (int q = 0; q < 9; ++q) o[q] = c.NN[((size_t)a * c.K + b) * 9 + q];
  } else {
    const double *t = c.NN + ((size_t)b * c.K + a) * 9;
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) o[r * 3 + q] = t[q * 3 + r];
  }
}
// Sigma(old variable at rows r0..r0+nr of Sigma, new pose b) = Sigma(., x_last) Fs_b^T   (nr x 3)
__device__ inline void cov_old_new(const Fm2Ctx &c, int r0, int nr, int b, double *o) {
  const double *fs = c.Fs + 9 * b;
  const int cl = 3 * (c.P - 1);
  for (int r = 0; r < nr; ++r) {
    const double *s = c.Sig + (size_t)(r0 + r) * c.n + cl;
    for (int q = 0; q < 3; ++q) o[r * 3 + q] = s[0] * fs[q * 3] + s[1] * fs[q * 3 + 1] + s[2] * fs[q * 3 + 2];
  }
}

// chain - thread 0 alone.  The odometry chain (FastMarginals.cpp:201-223), sequential over the new poses.
// Reads: the last pose's estimate and linearisation point, its block of Sig, the plan `act` [K][3].
// Leaves: newp, cov_new, F, Fs for b < K.
__device__ __forceinline__ void chain(const Fm2Ctx &c, const drlgx_config &cfg, const double *act) {
  const int P = c.P, n = c.n;
  Pose origin = pose_at(c.ep, P - 1);  // parent->state.pose (estimate)
  Pose val0 = pose_at(c.thp, P - 1);   // values.at(key0)
  double cov0[9], Fc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) cov0[r * 3 + q] = c.Sig[(size_t)(3 * (P - 1) + r) * n + 3 * (P - 1) + q];
  const double sg[3] = {cfg.translation_noise, cfg.translation_noise, cfg.rotation_noise};
  for (int b = 0; b < c.K; ++b) {
    Pose odom;
    const Pose end = chain_step(origin, act + 3 * b, &odom);
    c.newp[4 * b] = end.x; c.newp[4 * b + 1] = end.y; c.newp[4 * b + 2] = end.c; c.newp[4 * b + 3] = end.s;
    double H1b[9];
    const Pose hx = between(val0, end, H1b);
    const Pose h = between(odom, hx, nullptr);
    const double Hl[9] = {h.c, h.s, 0, -h.s, h.c, 0, 0, 0, 1};
    double A0[9], A1i[9];  // whitened block on key0; inverse of the whitened block on key1 (Hl is a rotation: Hl^-1 = Hl^T)
    mat3_mul(Hl, H1b, A0);
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) {
        A0[r * 3 + q] /= sg[r];
        A1i[r * 3 + q] = Hl[q * 3 + r] * sg[q];
      }
    double t1[9], t2[9], c1[9], fb[9], fsn[9];
    mat3_mul(A0, cov0, t1);
    mat3_mul_bt(t1, A0, t2);
    t2[0] += 1.0; t2[4] += 1.0; t2[8] += 1.0;
    mat3_mul(A1i, t2, t1);
    mat3_mul_bt(t1, A1i, c1);
    mat3_mul(A1i, A0, fb);
    for (int q = 0; q < 9; ++q) fb[q] = -fb[q];
    mat3_mul(fb, Fc, fsn);
    for (int q = 0; q < 9; ++q) {
      c.cov_new[9 * b + q] = c1[q];
      c.F[9 * b + q] = fb[q];
      c.Fs[9 * b + q] = fsn[q];
      Fc[q] = fsn[q];
      cov0[q] = c1[q];
    }
    origin = end;
    val0 = end;
  }
}

// cross - one thread per new pose a.  Reads cov_new, F.  Leaves NN(a, b) = Sigma(new a, new b) = cov_a F_{a+1}^T ... F_b^T, a <= b.
__device__ __forceinline__ void cross(const Fm2Ctx &c) {
  const int K = c.K;
  for (int a = threadIdx.x; a < K; a += kT) {
    double cur[9];
    for (int q = 0; q < 9; ++q) cur[q] = c.NN[((size_t)a * K + a) * 9 + q] = c.cov_new[9 * a + q];
    for (int b = a + 1; b < K; ++b) {
      double nx[9];
      mat3_mul_bt(cur, c.F + 9 * b, nx);
      for (int q = 0; q < 9; ++q) cur[q] = c.NN[((size_t)a * K + b) * 9 + q] = nx[q];
    }
  }
}

// predict - whole workgroup, with its own barriers (three per 256 landmarks of a core pose; every thread takes the same ones).
// The predicted measurements (Planner2D.cpp:717-731): new pose b x estimated landmark j, in (b, j) order.
// Reads newp, the landmarks' estimates and linearisation points; core_row ([K], kMask only): the steps that predict.
// Leaves: *nm_s = the number of measurements that pass the gates; mk, mj, J of the first min(*nm_s, nm_max) of them.
template <bool kMask>
__device__ __forceinline__ void predict(const Fm2Ctx &c, const drlgx_config &cfg, const uint8_t *core_row, int nm_max, int *nm_s, int *wcount) {
  const int tid = threadIdx.x, L = c.L;
  for (int b = 0; b < c.K; ++b) {
    if (kMask && !core_row[b]) continue;  // (the same for every thread: no barrier is left out by some)
    const Pose ps = pose_at(c.newp, b);
    for (int j0 = 0; j0 < L; j0 += kT) {
      const int j = j0 + tid;
      const bool ok = j < L && in_gate(cfg, ps, P2{c.el[2 * j], c.el[2 * j + 1]});
      // ordered compaction: wave ballots + a serial scan over the waves (4 waves)
      const unsigned long long bal = __ballot(ok);
      if ((tid & 63) == 0) wcount[tid >> 6] = __popcll(bal);
      __syncthreads();
      int base = *nm_s;
      for (int w = 0; w < (tid >> 6); ++w) base += wcount[w];
      const int idx = base + __popcll(bal & ((1ull << (tid & 63)) - 1ull));
      if (ok && idx < nm_max) {
        c.mk[idx] = b;
        c.mj[idx] = j;
        double Jx[6], Jl[4];
        br_jac(ps, P2{c.thl[2 * j], c.thl[2 * j + 1]}, Jx, Jl);  // landmark at its linearisation point
        double *o = c.J + (size_t)10 * idx;
        for (int q = 0; q < 3; ++q) {
          o[q] = Jx[q] / cfg.bearing_noise;
          o[3 + q] = Jx[3 + q] / cfg.range_noise;
        }
        o[6] = Jl[0] / cfg.bearing_noise; o[7] = Jl[1] / cfg.bearing_noise;
        o[8] = Jl[2] / cfg.range_noise; o[9] = Jl[3] / cfg.range_noise;
      }
      __syncthreads();
      if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < kT / 64; ++w) tot += wcount[w];
        *nm_s += tot;
      }
      __syncthreads();
    }
  }
}

// assemble_T - one thread per measurement pair (2x2 block).  Reads J, mk, mj, NN, Fs, Sig.  Leaves T = I + A Sigma_A A^T.
__device__ __forceinline__ void assemble_T(const Fm2Ctx &c) {
  const int P = c.P, n = c.n, nm = c.nm, dim = 2 * nm;
  for (int e = threadIdx.x; e < nm * nm; e += kT) {
    const int r = e / nm, s = e - r * nm;
    const double *jr = c.J + (size_t)10 * r, *js = c.J + (size_t)10 * s;
    const int kr = c.mk[r], ks = c.mk[s], lr = c.mj[r], ls = c.mj[s];
    double xx[9], xl[6], lx[6], ll[4];  // Sigma(x_kr, x_ks) 3x3, Sigma(x_kr, l_ls) 3x2, Sigma(l_lr, x_ks) 2x3, Sigma(l_lr, l_ls) 2x2
    cov_nn(c, kr, ks, xx);
    {
      double t[6];  // Sigma(l_ls, x_kr) (2x3) -> transpose
      cov_old_new(c, 3 * P + 2 * ls, 2, kr, t);
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 2; ++b) xl[a * 2 + b] = t[b * 3 + a];
    }
    cov_old_new(c, 3 * P + 2 * lr, 2, ks, lx);
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) ll[a * 2 + b] = c.Sig[(size_t)(3 * P + 2 * lr + a) * n + 3 * P + 2 * ls + b];
    // M = [Jx_r | Jl_r] [xx xl; lx ll] [Jx_s | Jl_s]^T
    double v[2][5];  // [Jx_r | Jl_r] * Sigma block: 2 x 5
    for (int a = 0; a < 2; ++a) {
      for (int q = 0; q < 3; ++q)
        v[a][q] = jr[3 * a] * xx[q] + jr[3 * a + 1] * xx[3 + q] + jr[3 * a + 2] * xx[6 + q] + jr[6 + 2 * a] * lx[q] + jr[7 + 2 * a] * lx[3 + q];
      for (int q = 0; q < 2; ++q)
        v[a][3 + q] = jr[3 * a] * xl[q] + jr[3 * a + 1] * xl[2 + q] + jr[3 * a + 2] * xl[4 + q] + jr[6 + 2 * a] * ll[q] + jr[7 + 2 * a] * ll[2 + q];
    }
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        const double m = v[a][0] * js[3 * b] + v[a][1] * js[3 * b + 1] + v[a][2] * js[3 * b + 2] + v[a][3] * js[6 + 2 * b] + v[a][4] * js[7 + 2 * b];
        c.T[(size_t)(2 * r + a) * dim + 2 * s + b] = m + ((r == s && a == b) ? 1.0 : 0.0);
      }
  }
}

// reduce_block<W> - one wave: U^T T^-1 U of one W-wide variable (a pose: 3, a landmark: 2), the upper triangle by rows.
// fill(r, u): a lane writes the two rows of measurement r, u[2][W] = (A Sigma(., variable))[2 r .. 2 r + 1].  Then lanes stride the rows
// of T^-1 U, then the shuffle tree; store(acc), lane 0: base - acc to where the block goes.  Both widths sum in this one order.
// Reads T (inverted), this wave's slab of U.  Wave barriers: after the fill (with its fences) and after the store.
template <int W, class Fill, class Store>
__device__ __forceinline__ void reduce_block(const Fm2Ctx &c, int lane, Fill fill, Store store) {
  constexpr int kAcc = W * (W + 1) / 2;
  const int dim = 2 * c.nm;
  double *U = c.U;
  for (int r = lane; r < c.nm; r += 64) fill(r, U + (size_t)2 * r * W);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  double acc[kAcc] = {};
  for (int r = lane; r < dim; r += 64) {
    double w[W] = {};  // (T^-1 U)[r][:]
    const double *tr = c.T + (size_t)r * dim;
    for (int s = 0; s < dim; ++s)
      for (int q = 0; q < W; ++q) w[q] += tr[s] * U[W * s + q];
    for (int a = 0, k = 0; a < W; ++a)
      for (int b = a; b < W; ++b) acc[k++] += U[W * r + a] * w[b];
  }
  for (int q = 0; q < kAcc; ++q)
    for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o);
  if (lane == 0) store(acc);
  __builtin_amdgcn_wave_barrier();
}

// One workgroup per candidate; its scratch: Fm2Scratch(S.A_max, nm_max) (fm2_carve.h), nm_max <= kFm2MaxMeas.
// kMask: `core` ([candidate][max_actions], the launch's first candidate first) marks the actions that are core poses; a non-core
// step - an intermediate pose of a Dubins edge (Planner2D.cpp:659-682) - gets its pose and its odometry factor like every action,
// and predicts no measurement.  kMask = false never reads `core`: every action is a core pose.
// kLm: the LANDMARK blocks as well (updateTrajectory_SLAM_OG_SHANNON, Planner2D.cpp:608-611, reads every landmark's marginal after
// the same update): lm_out [candidate][lm_stride][3] (xx, xy, yy per slot, the launch's first candidate first) gets
// Sigma'(l, l) = Sigma(l, l) - U_l^T T^-1 U_l, U_l = A Sigma(., l) (2 nm x 2), for the L slots of the candidate's environment; with no
// predicted measurement that is the prior block, bit for bit.  kLm = false never reads `lm_out` and is the kernel without them.
template <bool kMask, bool kLm>
__global__ __launch_bounds__(kT) void k_fm2_update(DrlgxState S, const int32_t *cand_env, const double *actions, const int32_t *n_actions,
                                                   const double *sig, size_t sig_stride, double *scratch, size_t scratch_stride,
                                                   int *iscratch, int nm_max, double *cov_out, int out_stride, int32_t *n_out,
                                                   const uint8_t *core, double *lm_out, int lm_stride) {
  __shared__ int nm_s, bad;
  __shared__ int wcount[kT / 64];
  __shared__ double gj[kGjDoubles];  // Gauss-Jordan column / row of T: dim = 2 nm <= 2 kFm2MaxMeas
  const int tid = threadIdx.x, ci = blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nw = kT / 64;
  const int env = cand_env[ci];
  const drlgx_config &cfg = S.cfg;
  const int *cnt = S.cnt + (size_t)env * DRLGX_CNT_STRIDE;
  const int P = cnt[C_P], L = cnt[C_L], K = n_actions[ci], n = 3 * P + 2 * L;
  const Fm2Scratch lay(S.A_max, nm_max);
  double *sc = scratch + (size_t)ci * scratch_stride;
  int *isc = iscratch + (size_t)ci * lay.itotal;
  const double *Sig = sig + (size_t)env * sig_stride;
  Fm2Ctx c{P, L, K, 0, Sig, n, sc + lay.cov_new, sc + lay.F, sc + lay.Fs, sc + lay.NN, isc + lay.mk, isc + lay.mj, sc + lay.J, sc + lay.T,
           sc + lay.U + (size_t)wave * lay.u_slab, sc + lay.newp,
           S.th_pose + (size_t)env * S.P_max * 4, S.th_lm + (size_t)env * S.L_max * 2,
           S.est_pose + (size_t)env * S.P_max * 4, S.est_lm + (size_t)env * S.L_max * 2};
  double *out = cov_out + (size_t)ci * out_stride * 9;
  if (tid == 0) {
    nm_s = 0;
    bad = 0;
    n_out[ci] = P + K;
    chain(c, cfg, actions + (size_t)ci * S.A_max * 3);
  }
  __syncthreads();
  cross(c);
  predict<kMask>(c, cfg, kMask ? core + (size_t)ci * S.A_max : nullptr, nm_max, &nm_s, wcount);
  if (nm_s > nm_max) {
    if (tid == 0) atomicMin(S.status, DRLGX_E_CAPACITY);
    return;
  }
  const int nm = c.nm = nm_s;
  assemble_T(c);
  __syncthreads();
  if (nm > 0) spd_inverse(c.T, 2 * nm, 2 * nm, gj, gj + kGjHalf, &bad);
  __syncthreads();
  // ---- every pose i: U_i = A Sigma(., x_i) (dim x 3), Sigma'_ii = Sigma_ii - U_i^T T^-1 U_i.  One wave per pose.
  for (int i = wave; i < P + K; i += nw)
    reduce_block<3>(
        c, lane,
        [&](int r, double *u) {
          const double *jr = c.J + (size_t)10 * r;
          const int kr = c.mk[r], lr = c.mj[r];
          double xi[9], li[6];  // Sigma(x_new kr, x_i) 3x3, Sigma(l_lr, x_i) 2x3
          if (i >= P) {
            cov_nn(c, kr, i - P, xi);
            cov_old_new(c, 3 * P + 2 * lr, 2, i - P, li);
          } else {
            double t[9];  // Sigma(x_i, x_new kr) -> transpose
            cov_old_new(c, 3 * i, 3, kr, t);
            for (int a = 0; a < 3; ++a)
              for (int b = 0; b < 3; ++b) xi[a * 3 + b] = t[b * 3 + a];
            for (int a = 0; a < 2; ++a)
              for (int b = 0; b < 3; ++b) li[a * 3 + b] = Sig[(size_t)(3 * P + 2 * lr + a) * n + 3 * i + b];
          }
          for (int a = 0; a < 2; ++a)
            for (int q = 0; q < 3; ++q)
              u[a * 3 + q] = jr[3 * a] * xi[q] + jr[3 * a + 1] * xi[3 + q] + jr[3 * a + 2] * xi[6 + q] + jr[6 + 2 * a] * li[q] + jr[7 + 2 * a] * li[3 + q];
        },
        [&](const double *acc) {
          double base[9];
          if (i >= P)
            for (int q = 0; q < 9; ++q) base[q] = c.cov_new[9 * (i - P) + q];
          else
            for (int r = 0; r < 3; ++r)
              for (int q = 0; q < 3; ++q) base[r * 3 + q] = Sig[(size_t)(3 * i + r) * n + 3 * i + q];
          double *o = out + (size_t)i * 9;
          // (the upper triangle, mirrored: the Gauss-Jordan prior and the chain's products are symmetric only up to round-off)
          o[0] = base[0] - acc[0]; o[1] = base[1] - acc[1]; o[2] = base[2] - acc[2];
          o[3] = o[1];             o[4] = base[4] - acc[3]; o[5] = base[5] - acc[4];
          o[6] = o[2];             o[7] = o[5];             o[8] = base[8] - acc[5];
        });
  // ---- every landmark l: U_l = A Sigma(., l) (dim x 2), Sigma'_ll = Sigma_ll - U_l^T T^-1 U_l.  One wave per landmark, through the
  // poses' reduce_block: the same candidate, the same bits.
  if (kLm) {
    double *lo = lm_out + (size_t)ci * lm_stride * 3;
    for (int l = wave; l < L; l += nw) {
      const int cl = 3 * P + 2 * l;
      reduce_block<2>(
          c, lane,
          [&](int r, double *u) {
            const double *jr = c.J + (size_t)10 * r;
            const int kr = c.mk[r], lr = c.mj[r];
            double t[6], ll[4];  // Sigma(l, x_new kr) 2x3 (its transpose is Sigma(x_new kr, l)), Sigma(l_lr, l) 2x2
            cov_old_new(c, cl, 2, kr, t);
            for (int a = 0; a < 2; ++a)
              for (int b = 0; b < 2; ++b) ll[a * 2 + b] = Sig[(size_t)(3 * P + 2 * lr + a) * n + cl + b];
            for (int a = 0; a < 2; ++a)
              for (int b = 0; b < 2; ++b)
                u[a * 2 + b] = jr[3 * a] * t[b * 3] + jr[3 * a + 1] * t[b * 3 + 1] + jr[3 * a + 2] * t[b * 3 + 2] + jr[6 + 2 * a] * ll[b] + jr[7 + 2 * a] * ll[2 + b];
          },
          [&](const double *acc) {
            lo[3 * l] = Sig[(size_t)cl * n + cl] - acc[0];
            lo[3 * l + 1] = Sig[(size_t)cl * n + cl + 1] - acc[1];
            lo[3 * l + 2] = Sig[(size_t)(cl + 1) * n + cl + 1] - acc[2];
          });
    }
  }
  if (tid == 0 && bad) atomicMin(S.status, DRLGX_E_NUMERIC);
}

// What k_fm2_update can only report through the status word, found out BEFORE anything is launched that an entry's caller could
// see: an environment that does not exist, a plan longer than max_actions, more predicted measurements than nm_max.  One thread
// per candidate walks k_fm2_update's pose chain and gates (chain_step, in_gate); flag[0] = the smallest DRLGX_E_* code met (the
// caller zeroes it).  kMask: k_fm2_update's mask - only core poses predict measurements, so only theirs count against nm_max;
// kMask = false never reads `core`.
template <bool kMask>
__global__ void k_fm2_check(DrlgxState S, int n_cand, const int32_t *cand_env, const double *actions, const int32_t *n_actions, int nm_max,
                            int *flag, const uint8_t *core) {
  const int ci = blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= n_cand) return;
  const int env = cand_env[ci], K = n_actions[ci];
  if (env < 0 || env >= S.n_envs || K < 0 || K > S.A_max) {
    atomicMin(flag, DRLGX_E_INVALID);
    return;
  }
  const int *cnt = S.cnt + (size_t)env * DRLGX_CNT_STRIDE;
  const int P = cnt[C_P], L = cnt[C_L];
  const double *el = S.est_lm + (size_t)env * S.L_max * 2;
  Pose origin = pose_at(S.est_pose + (size_t)env * S.P_max * 4, P - 1);
  int nm = 0;
  for (int b = 0; b < K; ++b) {
    Pose odom;
    const Pose ps = chain_step(origin, actions + ((size_t)ci * S.A_max + b) * 3, &odom);
    const int Lb = kMask && !core[(size_t)ci * S.A_max + b] ? 0 : L;
    for (int j = 0; j < Lb; ++j) nm += in_gate(S.cfg, ps, P2{el[2 * j], el[2 * j + 1]}) ? 1 : 0;
    origin = ps;
  }
  if (nm > nm_max) atomicMin(flag, DRLGX_E_CAPACITY);
}

}  // namespace kfm2

void drlgx_launch_fm2_check(const DrlgxState &S, hipStream_t st, int n_cand, const int32_t *cand_env, const double *actions,
                            const int32_t *n_actions, const uint8_t *core, int *flag) {
  const auto kernel = core ? kfm2::k_fm2_check<true> : kfm2::k_fm2_check<false>;
  hipLaunchKernelGGL(kernel, dim3((n_cand + 63) / 64), dim3(64), 0, st, S, n_cand, cand_env, actions, n_actions, kfm2::kFm2MaxMeas, flag, core);
}
void drlgx_launch_fm2_prior(const DrlgxState &S, hipStream_t st, double *sig, size_t sig_stride, int n_max) {
  hipLaunchKernelGGL(kfm2::k_fm2_prior, dim3(S.n_envs), dim3(kfm2::kT), 2 * (size_t)n_max * sizeof(double), st, S, sig, sig_stride);
}
void drlgx_launch_fm2_prior_ordered(const DrlgxState &S, hipStream_t st, double *sig, size_t sig_stride, int n_max) {
  hipLaunchKernelGGL(kfm2::k_fm2_prior_ordered, dim3(S.n_envs), dim3(kfm2::kT), 2 * (size_t)n_max * sizeof(double), st, S, sig, sig_stride);
}
size_t drlgx_fm2_scratch_doubles(const DrlgxState &S) { return kfm2::Fm2Scratch(S.A_max, kfm2::kFm2MaxMeas).total; }
void drlgx_launch_fm2_update(const DrlgxState &S, hipStream_t st, int nc, const int32_t *cand_env, const double *actions,
                             const int32_t *n_actions, const uint8_t *core, const double *sig, size_t sig_stride, double *scratch,
                             int *iscratch, double *cov_out, int out_stride, int32_t *n_out, double *lm_out, int lm_stride) {
#define DRLGX_FM2_UPDATE(kMask, kLm)                                                                                                 \
  hipLaunchKernelGGL((kfm2::k_fm2_update<kMask, kLm>), dim3(nc), dim3(kfm2::kT), 0, st, S, cand_env, actions, n_actions, sig, sig_stride, \
                     scratch, drlgx_fm2_scratch_doubles(S), iscratch, kfm2::kFm2MaxMeas, cov_out, out_stride, n_out, core, lm_out, lm_stride)
  if (core && lm_out) DRLGX_FM2_UPDATE(true, true);
  else if (core) DRLGX_FM2_UPDATE(true, false);
  else if (lm_out) DRLGX_FM2_UPDATE(false, true);
  else DRLGX_FM2_UPDATE(false, false);
#undef DRLGX_FM2_UPDATE
}
