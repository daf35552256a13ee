// Batched SLAM belief update, dense solver: one 512-thread workgroup per instance, the whole problem on chip.
// Holds SlamCtx (front / back), panel_from_dense, slam_finish, slam_body and the kernel k_slam; the fused step kernels
// (k_step.hip) run SlamCtx::front beside their simulator wave and slam_finish after it.
//
// Restates SLAM2D::optimize / copy_optimize (src/em_exploration/SLAM2D.cpp:374-488) — one iSAM2
// update (gtsam ISAM2::update, third-party; policy in SURVEY.md App. A.3) followed by the block
// marginals of FastMarginals (src/em_exploration/FastMarginals.cpp:130-186):
//   front end (SlamCtx::front; in k_step it runs beside the simulator wave, on the state before the step):
//   1. relinearisation policy (every 10th update, |delta|_inf >= 0.1), theta staged in LDS
//   2. every bearing-range factor is linearised ONCE by its own thread into a 12-double LDS record (linearize_br); landmark
//      2x2 blocks (thread per landmark, walking a bit mask of the observing poses), pose 3x3 blocks by roles: odometry
//      factors linearised once for both keys, own factors summed eight lanes per pose
//   back end (SlamCtx::back; after the simulator):
//   3. this step's factors; landmarks are eliminated analytically -> Schur complement S on the poses (3P x 3P, LDS)
//   4. symmetric Gauss-Jordan SWEEP of the augmented system [S rhs] on the fp64 matrix cores
//      (v_mfma_f64_16x16x4_f64): the lower triangle lives in 16 x 16 accumulator tiles in registers for the whole
//      factorisation; afterwards the triangle holds -S^-1 (every pose marginal and cross block) and the augmented row
//      holds delta_p.  sweep_packed_fast (k_sweep.hip; <= 53 poses, everything in LDS): 16-wide block pivots, one role per
//      wave (sweep_role), the next diagonal tile inverted in registers by an otherwise idle wave (inv16_blk).
//   5. landmark deltas and 2x2 landmark marginals by back-substitution through G = Lambda_pl Lambda_ll^-1
//   6. estimates theta (+) delta, information blocks (3x3 cofactor inverse / 2x2 inverse), traces
// LDS: the packed system + per-factor records when they fit; the records fall back to an HBM/L2 workspace otherwise.
// Trajectories beyond 53 poses (kDenseTiles): k_slam_arrow.hip (pose chain eliminated first).
#pragma once
#include "k_inc.hip"
namespace kslam {
#pragma clang fp contract(fast)
// The dense solver: <= 53 poses (N <= 16 kDenseTiles = 160), the whole problem in LDS.  Longer trajectories: arrow_body
// (k_slam_arrow.hip).
//
// The update is split in two so that the fused step kernel can run the first part BESIDE the simulator wave:
//   front  everything that does not depend on this step's measurements: relinearisation policy and theta staging,
//          linearisation of the factors that existed before the step, the pose blocks (the new pose's initial guess and
//          its odometry factor only depend on the commanded odometry and the previous estimate), the landmark sums over
//          the old factors.  In k_step it runs on 7 waves with software barriers (front<true>), in k_slam on all 8.
//   back   the new factors (linearisation, their terms appended to the sums in factor order - the same order of additions
//          as a single pass over all factors, so both kernels produce identical bits), landmark elimination, sweep, outputs.
static_assert(SlamCarve::kRec == REC, "slam_carve.h restates the record size");
constexpr bool slam_sys_matches_sweep() {
  for (size_t N = 16; N <= 16 * (size_t)kDenseTiles; N += 16)
    if (slam_sys_doubles(N) != sweep_region_doubles(N)) return false;
  return true;
}
static_assert(slam_sys_matches_sweep(), "slam_carve.h: the sweep region must be sweep_region_doubles (k_sweep.hip)");

// one bearing-range factor's terms of its landmark's block (a, b, d) and gradient (g0, g1), from the factor's record
__device__ __forceinline__ void lm_term_add(const double *r, double wb, double wr, double &a, double &b, double &d, double &g0, double &g1) {
  a += r[6] * wb * r[6] + r[8] * wr * r[8];
  b += r[6] * wb * r[7] + r[8] * wr * r[9];
  d += r[7] * wb * r[7] + r[9] * wr * r[9];
  g0 += r[6] * wb * r[10] + r[8] * wr * r[11];
  g1 += r[7] * wb * r[10] + r[9] * wr * r[11];
}
// The own bearing-range factors [m_begin, m_end) of one pose summed by eight adjacent lanes: lane `part` takes every eighth
// factor, the sums arrive in the lane with (lane & 7) == 7.  Whole waves call it (DPP sums), with an empty range where a lane
// group has no pose.
__device__ __forceinline__ void own_sum8(const double *rec, int m_begin, int m_end, int part, double wb, double wr, double (&s6)[6], double (&sg)[3]) {
  for (int q = 0; q < 6; ++q) s6[q] = 0.0;
  for (int r = 0; r < 3; ++r) sg[r] = 0.0;
  for (int m = m_begin + part; m < m_end; m += 8) own_factor_add(rec + (size_t)REC * m, wb, wr, s6, sg);
  for (int q = 0; q < 6; ++q) s6[q] = sum8_lane7(s6[q]);
  for (int r = 0; r < 3; ++r) sg[r] = sum8_lane7(sg[r]);
}
// butterfly sum of K values over the `split` (1, 2 or 4) adjacent lanes of a work item: DPP quad permutes, no trip through the
// LDS crossbar; a fixed tree, so deterministic
template <int K>
__device__ __forceinline__ void quad_butterfly(int split, double (&v)[K]) {
  if (split >= 4)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += dpp_quad_f64<0x4E>(v[k]);  // lane ^ 2
  if (split >= 2)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += dpp_quad_f64<0xB1>(v[k]);  // lane ^ 1
}

struct SlamCtx {
  int inst, P, L, M;     // poses of the system; landmarks / factors known so far (front) or final (back)
  int Lb, Mb;            // carve bounds of the per-landmark / per-factor arrays
  int np, N, Tn, MW;
  int n_old_p, n_old_l, count;
  bool relin;
  // LDS (the layout: slam_carve.h).  thl: the landmarks' linearisation points; from landmark_outputs on - when the map stage of
  // k_step reads them from LDS (`hand`) - their estimates (lm_estimates)
  double *thp, *odl, *thl, *lamb, *A, *rec;
  int *mstart, *bad, *lstart, *pstart;
  unsigned short *mp, *ml, *lfac, *obs, *pairlm;
  unsigned long long *lmask;

  __device__ __forceinline__ int AT(int i, int j) const { return i * (i + 1) / 2 + j; }
  // packed index of element t (xx, yx, yy, tx, ty, tt) of pose i's diagonal block; sigma_block: the six of them after the sweep,
  // negated (the triangle holds -Sigma_pp)
  __device__ __forceinline__ int sym3_index(int i, int t) const {
    const int r = t < 1 ? 0 : (t < 3 ? 1 : 2), cc = t - (r * (r + 1)) / 2;
    return AT(3 * i + r, 3 * i + cc);
  }
  __device__ __forceinline__ void sigma_block(int i, double (&s)[6]) const {
#pragma unroll
    for (int t = 0; t < 6; ++t) s[t] = -A[sym3_index(i, t)];
  }
  // bad[0]: set by a pivot that was not positive (inv16_blk), from clear_system to counters.
  __device__ __forceinline__ int &numeric_flag() const { return bad[0]; }
  // bad[1], three lives: the pairs of tile (0, 0) subtracted so far, from clear_system to the end of the Schur phase ...
  __device__ __forceinline__ int *pair_count() const { return bad + 1; }
  // ... and, after the sweep, the next work item of each of panel_from_dense's two item loops
  __device__ __forceinline__ int *work_counter() const { return bad + 1; }
  // the tables parked behind the packed triangle from pose_parts to pose_combine (SlamCarve::park_c2 / park_own)
  __device__ __forceinline__ double *c2buf() const { return A + SlamCarve::park_c2_doubles((size_t)N); }
  __device__ __forceinline__ double *ownsum() const { return A + SlamCarve::park_own_doubles((size_t)N, (size_t)P); }
  // thl once `back` ran with `hand`: the landmark estimates, left in LDS for the map stage
  __device__ __forceinline__ const double *lm_estimates() const { return thl; }

  // LDS carve from byte offset `off` of the dynamic shared memory (SlamCarve): small arrays first, then the dense system, then -
  // kBigLds - the factor records and the observation table, which otherwise go to the HBM workspace
  __device__ __forceinline__ static bool big_fits(size_t off, int lds_bytes, int P, int Lb, int Mb) {
    return SlamCarve(P, Lb, Mb, off).with_records <= (size_t)lds_bytes;
  }
  template <bool kBigLds>
  __device__ __forceinline__ void setup(const DrlgxState &S, unsigned char *smem_raw, size_t off, int lds_bytes, int inst_, int P_, int Lb_, int Mb_) {
    inst = inst_; P = P_; Lb = Lb_; Mb = Mb_;
    const SlamCarve cv(P, Lb, Mb, off);  // (transient: the context is copied and lives across the simulator wave)
    // padded to 16x16 MFMA tiles; row np holds the rhs (its column and all pad rows / columns stay zero).  Only the lower
    // triangle is ever addressed and it is stored packed (row i at i (i + 1) / 2)
    np = cv.np; Tn = cv.Tn; N = cv.N; MW = cv.MW;
    thp = reinterpret_cast<double *>(smem_raw + cv.thp);
    odl = reinterpret_cast<double *>(smem_raw + cv.odl);
    thl = reinterpret_cast<double *>(smem_raw + cv.thl);
    lamb = reinterpret_cast<double *>(smem_raw + cv.lamb);
    mstart = reinterpret_cast<int *>(smem_raw + cv.mstart);
    lstart = reinterpret_cast<int *>(smem_raw + cv.lstart);
    pstart = reinterpret_cast<int *>(smem_raw + cv.pstart);
    mp = reinterpret_cast<unsigned short *>(smem_raw + cv.mp);
    ml = reinterpret_cast<unsigned short *>(smem_raw + cv.ml);
    lfac = reinterpret_cast<unsigned short *>(smem_raw + cv.lfac);
    pairlm = reinterpret_cast<unsigned short *>(smem_raw + cv.pairlm);
    bad = reinterpret_cast<int *>(smem_raw + cv.bad);
    lmask = reinterpret_cast<unsigned long long *>(smem_raw + cv.lmask);
    A = reinterpret_cast<double *>(smem_raw + cv.sys);
    if constexpr (kBigLds) {
      rec = reinterpret_cast<double *>(smem_raw + cv.rec);
      obs = reinterpret_cast<unsigned short *>(smem_raw + cv.obs);
    } else {
      double *wsd = S.slam_ws + (size_t)inst * S.slam_ws_stride;
      rec = wsd; wsd += (size_t)S.M_max * REC;
      obs = reinterpret_cast<unsigned short *>(wsd);
    }
    // Both are used through `flat` instructions whatever their placement: with pointers the compiler knows to be LDS the
    // record-walking phases measured SLOWER (landmark marginals 3.9 -> 6.6 us, the loads are scheduled as short-latency
    // ones), so the address space is hidden from it
    asm volatile("" : "+v"(rec));
    asm volatile("" : "+v"(obs));
  }

  // ================================ front end: its phases.  t / nt: the caller's index among the threads that run it ================================
  // 1. relinearisation policy (gtsam ISAM2: relinearizeSkip 10, relinearizeThreshold 0.1); theta (+ folded delta) is staged in
  //    LDS, under kSub with the pose that this step appends
  template <bool kSub>
  __device__ __forceinline__ void stage_theta(const DrlgxState &S, int t, int nt, int Pf, int Lf, const double *odom3) const {
    double *th_pose = S.th_pose + (size_t)inst * S.P_max * 4;
    double *d_pose = S.d_pose + (size_t)inst * S.P_max * 3;
    double *th_lm = S.th_lm + (size_t)inst * S.L_max * 2;
    double *d_lm = S.d_lm + (size_t)inst * S.L_max * 2;
    for (int i = t; i < Pf; i += nt) {
      Pose th{th_pose[4 * i], th_pose[4 * i + 1], th_pose[4 * i + 2], th_pose[4 * i + 3]};
      if (relin && i < n_old_p) {
        const double a = fabs(d_pose[3 * i]), b = fabs(d_pose[3 * i + 1]), c = fabs(d_pose[3 * i + 2]);
        if (fmax(a, fmax(b, c)) >= 0.1) {
          th = compose(th, make_pose(d_pose[3 * i], d_pose[3 * i + 1], d_pose[3 * i + 2]));
          th_pose[4 * i] = th.x; th_pose[4 * i + 1] = th.y; th_pose[4 * i + 2] = th.c; th_pose[4 * i + 3] = th.s;
        }
      }
      thp[4 * i] = th.x; thp[4 * i + 1] = th.y; thp[4 * i + 2] = th.c; thp[4 * i + 3] = th.s;
      if (i + 1 < Pf) {  // measured odometry between pose i and i + 1
        const double *oo = S.odo + ((size_t)inst * S.P_max + i) * 4;
        odl[4 * i] = oo[0]; odl[4 * i + 1] = oo[1]; odl[4 * i + 2] = oo[2]; odl[4 * i + 3] = oo[3];
      }
    }
    if constexpr (kSub) {
      // the pose this step appends: SLAM2D::addOdometry's initial guess = last estimate * odom (SLAM2D.cpp:70-89), the same
      // expressions as the simulator wave evaluates (k_sim.hip sim_step_body), which stores them to HBM
      if (t == nt - 1) {
        const Pose odomP = make_pose(odom3[0], odom3[1], odom3[2]);
        const double *ep = S.est_pose + ((size_t)inst * S.P_max + (Pf - 1)) * 4;
        const Pose p2 = compose(Pose{ep[0], ep[1], ep[2], ep[3]}, odomP);
        thp[4 * Pf] = p2.x; thp[4 * Pf + 1] = p2.y; thp[4 * Pf + 2] = p2.c; thp[4 * Pf + 3] = p2.s;
        odl[4 * (Pf - 1)] = odomP.x; odl[4 * (Pf - 1) + 1] = odomP.y; odl[4 * (Pf - 1) + 2] = odomP.c; odl[4 * (Pf - 1) + 3] = odomP.s;
      }
    }
    for (int j = t; j < Lf; j += nt) {
      double x = th_lm[2 * j], y = th_lm[2 * j + 1];
      if (relin && j < n_old_l && fmax(fabs(d_lm[2 * j]), fabs(d_lm[2 * j + 1])) >= 0.1) {
        x += d_lm[2 * j];
        y += d_lm[2 * j + 1];
        th_lm[2 * j] = x;
        th_lm[2 * j + 1] = y;
      }
      thl[2 * j] = x;
      thl[2 * j + 1] = y;
    }
  }
  // 2. the system, the observation table and masks, the factor ranges and the two words of `bad` start empty
  __device__ __forceinline__ void clear_system(int t, int nt) const {
    double2 *A2 = reinterpret_cast<double2 *>(A);
    const int n2 = (int)((size_t)N * (N + 1) / 2 / 2);  // (N is a multiple of 16: even)
    for (int e = t; e < n2; e += nt) A2[e] = make_double2(0.0, 0.0);
    for (int e = t; e < Lb * P; e += nt) obs[e] = 0;
    for (int e = t; e < MW * Lb; e += nt) lmask[e] = 0ull;
    for (int e = t; e <= P; e += nt) mstart[e] = 0x7fffffff;
    if (t == 0) {
      numeric_flag() = 0;
      *pair_count() = 0;
    }
  }
  // tables + the (expensive) linearisation of the factors [m0, m1), one thread each (factors are appended in pose order:
  // contiguous ranges)
  __device__ __forceinline__ void factor_tables(const DrlgxState &S, int m0, int m1, int t, int nt, const SimBox &box = SimBox{nullptr, nullptr, nullptr}) const {
    const int *meas_pose = S.meas_pose + (size_t)inst * S.M_max;
    const int *meas_lm = S.meas_lm + (size_t)inst * S.M_max;
    const double *meas_br = S.meas_br + (size_t)inst * S.M_max * 2;
    if (box.br) {  // this step's factors from the simulator wave's LDS: all of them observed from the newest pose
      const int p = P - 1;
      for (int m = m0 + t; m < m1; m += nt) {
        const int j = box.slot[m - m0];
        mp[m] = (unsigned short)p;
        ml[m] = (unsigned short)j;
        if (m == m0) mstart[p] = m;
        obs[j * P + p] = (unsigned short)(m + 1);
        atomicOr(&lmask[MW * j + (p >> 6)], 1ull << (p & 63));
        linearize_br(thp + 4 * p, thl + 2 * j, box.br[2 * (m - m0)], box.br[2 * (m - m0) + 1], rec + (size_t)REC * m);
      }
      return;
    }
    for (int m = m0 + t; m < m1; m += nt) {
      const int p = meas_pose[m], j = meas_lm[m];
      mp[m] = (unsigned short)p;
      ml[m] = (unsigned short)j;
      if (m == 0 || meas_pose[m - 1] != p) mstart[p] = m;
      obs[j * P + p] = (unsigned short)(m + 1);
      atomicOr(&lmask[MW * j + (p >> 6)], 1ull << (p & 63));
      linearize_br(thp + 4 * p, thl + 2 * j, meas_br[2 * m], meas_br[2 * m + 1], rec + (size_t)REC * m);
    }
  }
  // poses without factors get the empty range [next pose's start, same): the first assigned start at or after p, i.e.
  // the suffix minimum of the raw starts (they increase with the pose); one wave (t < 64), top chunk first
  __device__ __forceinline__ void fill_mstart(int t, int Mf) const {
    if (t >= 64) return;
    int carry = 0x7fffffff;
    for (int base = (P >> 6) << 6; base >= 0; base -= 64) {
      const int q = base + t;
      int v = q < P ? mstart[q] : (q == P ? Mf : 0x7fffffff);  // (the end of the list = the start of this step's factors)
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int w = __shfl_down(v, o);
        if (t + o < 64) v = min(v, w);
      }
      v = min(v, carry);
      if (q <= P) mstart[q] = v;
      carry = __shfl(v, 0);
    }
  }
  // 3. block assembly.  Landmark blocks: one thread per landmark over the old factors (back() appends this step's terms)
  __device__ __forceinline__ void landmark_sums(const DrlgxState &S, int t, int nt) const {
    const double wb = S.w_bear, wr = S.w_range;
    for (int j = t; j < L; j += nt) {
      double a = 0, b = 0, d = 0, g0 = 0, g1 = 0;
      FOR_EACH_OBSERVING_POSE(lmask + MW * j, MW, p) lm_term_add(rec + (size_t)REC * (obs[j * P + p] - 1), wb, wr, a, b, d, g0, g1);
      double *lb = lamb + 8 * j;
      lb[0] = a; lb[1] = b; lb[2] = d; lb[3] = g0; lb[4] = g1;
    }
  }
  // Pose blocks (pose_block in pieces).  The LAST wave (la = t - (nt - 64) >= 0): lane i linearises odometry factor i once - for
  // both of its keys - and lane P - 1, which has none, the prior; the contributions to the second key travel through LDS
  // (c2buf, 9 doubles per pose; slot 0 = the prior), those to the first stay in B6 / g3.  The threads below it, eight per pose
  // from the top down (the landmark loop above occupies the first ones): the own bearing-range factors, every eighth factor
  // per lane, summed over the eight lanes into ownsum (back() adds the newest pose's the same way when this front end ran
  // before they existed: both ways round alike).
  __device__ __forceinline__ void pose_parts(const DrlgxState &S, int t, int nt, int lane, double (&B6)[6], double (&g3)[3]) const {
    const double wb = S.w_bear, wr = S.w_range;
    const int la = t - (nt - 64);
    if (la >= 0) {
      if (la + 1 < P) {
        double C2[6], g2[3], O[9];
        odo_factor(S, thp, odl, la, B6, g3, C2, g2, O);
        double *o2 = c2buf() + 9 * (la + 1);
        for (int q = 0; q < 6; ++q) o2[q] = C2[q];
        for (int r = 0; r < 3; ++r) o2[6 + r] = g2[r];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) A[AT((3 * (la + 1) + r), 3 * la + c)] = O[r * 3 + c];
      } else if (la == P - 1) {
        double PB[6], pg[3];
        prior_factor(S, inst, thp, PB, pg);
        double *o2 = c2buf();
        for (int q = 0; q < 6; ++q) o2[q] = PB[q];
        for (int r = 0; r < 3; ++r) o2[6 + r] = pg[r];
      }
    } else {
      const int idx = nt - 65 - t, grp = idx >> 3, part = idx & 7, ngrp = (nt - 64) >> 3;
      for (int i0 = 0; i0 < P; i0 += ngrp) {  // (uniform trip count: the lane sums run on whole waves)
        const int i = i0 + grp;
        int m_begin = 0, m_end = 0;
        if (i < P) {
          m_begin = mstart[i];
          m_end = mstart[i + 1];
        }
        double s6[6], sg[3];
        own_sum8(rec, m_begin, m_end, part, wb, wr, s6, sg);
        if (i < P && (lane & 7) == 7) {
          double *o = ownsum() + 9 * i;
          for (int q = 0; q < 6; ++q) o[q] = s6[q];
          for (int r = 0; r < 3; ++r) o[6 + r] = sg[r];
        }
      }
    }
  }
  // ... and, a barrier later, lane i of the last wave adds pose i's three parts in the order pose_block adds them: prior / second
  // key, first key, own factors
  __device__ __forceinline__ void pose_combine(int t, int nt, const double (&B6)[6], const double (&g3)[3]) const {
    const int la = t - (nt - 64);
    if (la < 0 || la >= P) return;
    const double *c2 = c2buf() + 9 * la, *own = ownsum() + 9 * la;
    double B[6], g[3];
    for (int q = 0; q < 6; ++q) B[q] = (c2[q] + B6[q]) + own[q];
    for (int r = 0; r < 3; ++r) g[r] = (c2[6 + r] + g3[r]) + own[6 + r];
    for (int r = 0, q = 0; r < 3; ++r) {
      for (int c = 0; c <= r; ++c, ++q) A[AT((3 * la + r), 3 * la + c)] = B[q];
      A[AT(np, 3 * la + r)] = -g[r];  // rhs lives in the augmented row
    }
  }

  // kSub: called by the threads 64 .. kThreads-1 (ft = tid - 64) while wave 0 simulates; Pf / L / M are the counts before
  // the step, the new pose (index Pf) comes from `odomP`.  Otherwise by all threads with the final counts (Pf = P).
  template <bool kSub>
  __device__ __forceinline__ void front(const DrlgxState &S, int tid, int Pf, int Lf, int Mf, int n_old_p_, int n_old_l_, int count_,
                                        bool refresh, const double *odom3, SubBarrier sb) {
    const int ft = kSub ? tid - 64 : tid, fn = kSub ? kThreads - 64 : kThreads, lane = tid & 63;
    auto bar = [&]() {
      if constexpr (kSub) sb.sync(lane);
      else __syncthreads();
    };
    auto mark = [&](int slot) {
      if (S.prof && blockIdx.x == S.prof_block && ft == 0) S.prof[slot] = wall_clock64();
    };
    L = Lf; M = Mf; n_old_p = n_old_p_; n_old_l = n_old_l_; count = count_;
    relin = !refresh && (count % 10 == 0);
    stage_theta<kSub>(S, ft, fn, Pf, Lf, odom3);
    clear_system(ft, fn);
    bar();
    mark(33);
    factor_tables(S, 0, Mf, ft, fn);
    bar();
    mark(34);
    fill_mstart(ft, Mf);
    bar();
    mark(35);
    landmark_sums(S, ft, fn);
    double B6[6] = {0, 0, 0, 0, 0, 0}, g3[3] = {0, 0, 0};
    pose_parts(S, ft, fn, lane, B6, g3);
    bar();
    pose_combine(ft, fn, B6, g3);
    mark(14);  // (dev aid: end of the front end, first thread and per wave)
    if (S.prof && blockIdx.x == S.prof_block && lane == 0) S.prof[24 + (tid >> 6)] = wall_clock64();
  }

  // ================================ back end: its phases, all kThreads threads ================================
  // this step's landmarks (all of them observed from the newest pose); its factors: factor_tables, a barrier later
  __device__ __forceinline__ void append_step(const DrlgxState &S, int tid, int L0, const SimBox &box) const {
    const double *th_lm = S.th_lm + (size_t)inst * S.L_max * 2;
    for (int j = L0 + tid; j < L; j += kThreads) {
      thl[2 * j] = box.br ? box.lm[2 * (j - L0)] : th_lm[2 * j];
      thl[2 * j + 1] = box.br ? box.lm[2 * (j - L0) + 1] : th_lm[2 * j + 1];
      double *lb = lamb + 8 * j;
      lb[0] = lb[1] = lb[2] = lb[3] = lb[4] = 0.0;
    }
    if (tid == 0) mstart[P] = M;
  }
  // landmark blocks: this step's term (at most one per landmark) closes the sum, then Lambda_jj^-1 and eta_j; CSR offsets of
  // the per-landmark factor lists (the last wave); the newest pose's own factors close its block (one group of eight lanes)
  __device__ __forceinline__ void close_landmarks(const DrlgxState &S, int tid, int M0) const {
    const double wb = S.w_bear, wr = S.w_range;
    for (int j = tid; j < L; j += kThreads) {
      double *lb = lamb + 8 * j;
      double a = lb[0], b = lb[1], d = lb[2], g0 = lb[3], g1 = lb[4];
      const int m1 = M > M0 ? obs[j * P + (P - 1)] : 0;
      if (m1 > M0) lm_term_add(rec + (size_t)REC * (m1 - 1), wb, wr, a, b, d, g0, g1);
      const double id = 1.0 / (a * d - b * b);
      lb[0] = a; lb[1] = b; lb[2] = d;
      lb[3] = d * id; lb[4] = -b * id; lb[5] = a * id;  // Lambda_jj^-1
      lb[6] = -g0; lb[7] = -g1;                           // eta_j
    }
    if (tid >= kThreads - 64) {  // exclusive scan of the observation counts -> lstart[0 .. L]
      const int ln = tid - (kThreads - 64);
      unsigned carry = 0;
      for (int base = 0; base < L; base += 64) {
        const int j = base + ln;
        int k = 0;
        if (j < L)
          for (int w = 0; w < MW; ++w) k += __popcll(lmask[MW * j + w]);
        // (two scans in one: observations in the low half, pairs of observations - ceil(k / 2) - in the high half)
        const int k2 = (k + 1) >> 1;
        unsigned v = (unsigned)k | ((unsigned)k2 << 16);
        // inclusive scan over the wave on DPP: row shifts inside the 16-lane rows, then the two row broadcasts
        v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
        v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
        v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
        v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8
        v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true);  // row_bcast:15 -> rows 1, 3
        v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true);  // row_bcast:31 -> rows 2, 3
        if (j < L) {
          lstart[j] = (int)((carry & 0xffffu) + (v & 0xffffu)) - k;
          pstart[j] = (int)((carry >> 16) + (v >> 16)) - k2;
        }
        carry += (unsigned)__builtin_amdgcn_readlane((int)v, 63);
      }
      if (ln == 0) {
        lstart[L] = (int)(carry & 0xffffu);
        pstart[L] = (int)(carry >> 16);
      }
    }
    if (M > M0 && (tid >> 3) == kThreads / 16) {
      // the own factors of the newest pose, appended after the front ran: eight lanes, every eighth factor each, like the
      // front end sums the own factors of every pose (so that (front + this) == the front alone when it runs after them)
      const int i = P - 1;
      double s6[6], sg[3];
      own_sum8(rec, M0, M, 7 - (tid & 7), wb, wr, s6, sg);
      if ((tid & 7) == 7) {
        for (int r = 0, q = 0; r < 3; ++r) {
          for (int c = 0; c <= r; ++c, ++q) A[AT(3 * i + r, 3 * i + c)] += s6[q];
          A[AT(np, 3 * i + r)] = -(-A[AT(np, 3 * i + r)] + sg[r]);
        }
      }
    }
  }
  // 4. landmark elimination: rec[0..5] <- G_m = Lambda_pl Lambda_ll^-1 (3x2), rec[6..11] <- H_m = G_m Lambda_jj
  //    (= Lambda_pl; the Jacobian of the landmark and the residual are not needed any more);
  //    per-landmark factor lists lfac[lstart[j] ..] in pose order, and the pair table of phase 6
  __device__ __forceinline__ void eliminate_landmarks(const DrlgxState &S, int tid) const {
    const double wb = S.w_bear, wr = S.w_range;
    for (int m = tid; m < M; m += kThreads) {
      double *l = rec + (size_t)REC * m;
      const double *lb = lamb + 8 * ml[m];
      double g[6], h[6];
      for (int r = 0; r < 3; ++r) {
        const double b0 = l[r] * wb * l[6] + l[3 + r] * wr * l[8];
        const double b1 = l[r] * wb * l[7] + l[3 + r] * wr * l[9];
        g[r * 2 + 0] = b0 * lb[3] + b1 * lb[4];
        g[r * 2 + 1] = b0 * lb[4] + b1 * lb[5];
      }
      for (int r = 0; r < 3; ++r) {
        h[r * 2 + 0] = g[r * 2] * lb[0] + g[r * 2 + 1] * lb[1];
        h[r * 2 + 1] = g[r * 2] * lb[1] + g[r * 2 + 1] * lb[2];
      }
      for (int k = 0; k < 6; ++k) l[k] = g[k];
      for (int k = 0; k < 6; ++k) l[6 + k] = h[k];
      // the factor's place in its landmark's list = the rank of its pose among the observers (no list walk)
      const int j = ml[m], p = mp[m];
      int rank = 0;
      for (int w = 0; w < (p >> 6); ++w) rank += __popcll(lmask[MW * j + w]);
      rank += __popcll(lmask[MW * j + (p >> 6)] & ((1ull << (p & 63)) - 1ull));
      lfac[lstart[j] + rank] = (unsigned short)m;
      if (rank < pstart[j + 1] - pstart[j]) pairlm[pstart[j] + rank] = (unsigned short)j;
    }
  }
  //    Schur complement: S_pq -= sum_j G_m Lambda_jj G_mq^T   (Lambda_pl = G Lambda_jj = H)
  // While the other seven waves do that, the wave that inverts the diagonal tiles in the sweep (an idle tile row's wave
  // when the system has fewer than FT tile rows - pre_e0: <= 37 poses) already inverts the FIRST one: tile (0, 0) is complete as
  // soon as the pairs of the poses 0..5 are subtracted - the first 21 pairs, counted in pair_count by their threads -
  // and its inversion (2.2 us) used to run after this phase with every other wave waiting at a barrier.  Returns E_0 in that wave.
  template <int FT>
  __device__ __forceinline__ v4d schur(const DrlgxState &S, int tid, bool pre_e0) const {
    const int ewave_first = 64 * (FT / 2);  // first thread of that wave (sweep_packed_fast: wave FT / 2 owns tile row FT - 1)
    const bool is_ewave = pre_e0 && tid >= ewave_first && tid < ewave_first + 64;
    v4d e0 = {0.0, 0.0, 0.0, 0.0};
    if (is_ewave) {
      const int p6 = min(P, 6), need = p6 * (p6 + 1) / 2;
      while (__hip_atomic_load(pair_count(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(2);
      __threadfence_block();
      const int lane = tid & 63, lc = lane & 15, lr = lane >> 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = lr + 4 * r;
        e0[r] = A[AT(max(i, lc), min(i, lc))];  // (N >= 16: the whole tile is inside the triangle)
      }
      const SweepCtx x{FT - 1, lane, lc, lr, np, N, false, true, bad, nullptr};
      inv16_blk(x, min(16, np), e0);
      return e0;
    }
    const int npairs = P * (P + 1) / 2;
    const int sidx = (pre_e0 && tid >= ewave_first) ? tid - 64 : tid, sn = pre_e0 ? kThreads - 64 : kThreads;
    for (int e = sidx; e < npairs; e += sn) {
      int p = (int)((sqrtf(8.0f * e + 1.0f) - 1.0f) * 0.5f);
      while ((p + 1) * (p + 2) / 2 <= e) ++p;
      while (p * (p + 1) / 2 > e) --p;
      const int q = e - p * (p + 1) / 2;
      // Row-major pairs: the lanes of a wave share p (one factor list, one trip count).  Measured and dropped - none
      // faster than this plain loop (5.2 us; 9.1 us for the instances with the most factors, of which 2.1 / 4.3 us are
      // the look-ups and the rest the terms): four look-ups per round issued together; look-ups software-pipelined one
      // factor ahead; the landmarks common to both poses from per-pose bit masks; diagonal-major pair order (lanes of
      // similar hit counts, but different factor lists: 6.2 / 9.8 us); two lanes per pair on the even / odd factors with a
      // DPP sum (three rounds of half the length instead of 1.3 of the full one: 6.9 / 9.9 us - the per-pair overhead,
      // index decode and the nine read-modify-writes, is worth ~2.5 loop iterations).
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      bool any = false;
      for (int m = mstart[p]; m < mstart[p + 1]; ++m) {
        const int mq1 = obs[ml[m] * P + q];
        if (!mq1) continue;
        any = true;
        const double *h = rec + (size_t)REC * m + 6, *gq = rec + (size_t)REC * (mq1 - 1);
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) acc[r * 3 + c] += h[r * 2] * gq[c * 2] + h[r * 2 + 1] * gq[c * 2 + 1];
      }
      if (any)
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            if (p == q && c > r) continue;
            A[AT((3 * p + r), 3 * q + c)] -= acc[r * 3 + c];
          }
      if (pre_e0 && p < 6) {  // a pair of tile (0, 0): done (release: the subtractions above are visible before the count)
        __threadfence_block();
        atomicAdd(pair_count(), 1);
      }
    }
    for (int p = (tid + kThreads - 64 * (FT / 2 + 1)) % kThreads; p < P; p += kThreads) {  // rhs_p -= sum_m G_m eta_j (idle waves)
      double s0 = 0, s1 = 0, s2 = 0;
      for (int m = mstart[p]; m < mstart[p + 1]; ++m) {
        const double *g = rec + (size_t)REC * m, *lb = lamb + 8 * ml[m];
        s0 += g[0] * lb[6] + g[1] * lb[7];
        s1 += g[2] * lb[6] + g[3] * lb[7];
        s2 += g[4] * lb[6] + g[5] * lb[7];
      }
      A[AT(np, 3 * p + 0)] -= s0;
      A[AT(np, 3 * p + 1)] -= s1;
      A[AT(np, 3 * p + 2)] -= s2;
    }
    return e0;
  }
  // 6. landmark marginals: Sigma_jj = Lambda_jj^-1 + sum_{a, b} G_a^T Sigma[p_a][p_b] G_b over the landmark's factor list
  //    (ascending poses).  By symmetry only b <= a is evaluated: factor a gets
  //        rec[6..9] <- Y_a + X_a + X_a^T,   Y_a = G_a^T Sigma_aa G_a,   X_a = sum_{b < a} G_a^T Sigma_ab G_b,
  //    whose sum over the list is the full double sum.  One work item = the list entries a and k-1-a of a landmark
  //    (a + (k-1-a) = k-1 block products whatever a: balanced), split over S6 adjacent lanes and combined by a
  //    butterfly.  The longest list sets the latency of this phase: (k-1) / S6 rounds.
  __device__ __forceinline__ void landmark_marginals(int tid) const {
    const int NP = pstart[L];
    const int sh6 = 4 * NP <= kThreads ? 2 : 2 * NP <= kThreads ? 1 : 0, S6 = 1 << sh6;
    const int per_pass = kThreads >> sh6;
    for (int pid0 = 0; pid0 < NP; pid0 += per_pass) {
      const int pid = pid0 + (tid >> sh6), s6 = tid & (S6 - 1);
      const bool work = pid < NP;
      double X[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // X_a of the two entries (each row major 2 x 2)
      int ma[2] = {0, 0};
      bool two = false;
      if (work) {
        const int j = pairlm[pid], t0 = lstart[j], k = lstart[j + 1] - t0;
        const int a0 = pid - pstart[j], a1 = k - 1 - a0;  // a0 <= a1
        two = a1 > a0;
        ma[0] = lfac[t0 + a0];
        ma[1] = lfac[t0 + a1];
        const int pa0 = mp[ma[0]], pa1 = mp[ma[1]];
        double W[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
        // the earlier entries b of the list: Sigma[p_a][p_b] = -(swept block), stored as rows of the later pose p_a
        for (int b = s6; b < a1; b += S6) {
          const int mb = lfac[t0 + b], pb = mp[mb];
          const double *gb = rec + (size_t)REC * mb;
          const double g0 = gb[0], g1 = gb[1], g2 = gb[2], g3 = gb[3], g4 = gb[4], g5 = gb[5];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            if (e == 0 && (b >= a0 || !two)) continue;
            const int pa = e ? pa1 : pa0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
              const int row = AT(3 * pa + r, 3 * pb);
              const double t0v = A[row], t1v = A[row + 1], t2v = A[row + 2];
              W[e][r * 2] -= t0v * g0 + t1v * g2 + t2v * g4;
              W[e][r * 2 + 1] -= t0v * g1 + t1v * g3 + t2v * g5;
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const double *ga = rec + (size_t)REC * ma[e];
          X[4 * e + 0] = ga[0] * W[e][0] + ga[2] * W[e][2] + ga[4] * W[e][4];
          X[4 * e + 1] = ga[0] * W[e][1] + ga[2] * W[e][3] + ga[4] * W[e][5];
          X[4 * e + 2] = ga[1] * W[e][0] + ga[3] * W[e][2] + ga[5] * W[e][4];
          X[4 * e + 3] = ga[1] * W[e][1] + ga[3] * W[e][3] + ga[5] * W[e][5];
        }
      }
      quad_butterfly(S6, X);
      if (work && s6 == 0) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (e == 0 && !two) continue;  // (a0 == a1: the middle entry of an odd list, handled as e = 1)
          double *g = rec + (size_t)REC * ma[e];
          // Y = G^T Sigma_aa G with the symmetric diagonal block s = (s00, s10, s11, s20, s21, s22)
          double s[6];
          sigma_block(mp[ma[e]], s);
          const double d00 = s[0] * g[0] + s[1] * g[2] + s[3] * g[4], d01 = s[0] * g[1] + s[1] * g[3] + s[3] * g[5];
          const double d10 = s[1] * g[0] + s[2] * g[2] + s[4] * g[4], d11 = s[1] * g[1] + s[2] * g[3] + s[4] * g[5];
          const double d20 = s[3] * g[0] + s[4] * g[2] + s[5] * g[4], d21 = s[3] * g[1] + s[4] * g[3] + s[5] * g[5];
          const double y00 = g[0] * d00 + g[2] * d10 + g[4] * d20, y01 = g[0] * d01 + g[2] * d11 + g[4] * d21;
          const double y10 = g[1] * d00 + g[3] * d10 + g[5] * d20, y11 = g[1] * d01 + g[3] * d11 + g[5] * d21;
          g[6] = y00 + 2.0 * X[4 * e + 0];
          g[7] = y01 + (X[4 * e + 1] + X[4 * e + 2]);
          g[8] = y10 + (X[4 * e + 1] + X[4 * e + 2]);
          g[9] = y11 + 2.0 * X[4 * e + 3];
        }
      }
    }
  }
  // landmark deltas, estimates, marginals' traces and information blocks.  A landmark's list is split over S7 adjacent lanes - the
  // first half of the workgroup; pose_outputs takes the second - and combined by a butterfly.  With `hand`, thl becomes lm_estimates
  __device__ __forceinline__ void landmark_outputs(const DrlgxState &S, int tid, bool full, bool hand) const {
    double *d_lm = S.d_lm + (size_t)inst * S.L_max * 2;
    double *est_lm = S.est_lm + (size_t)inst * S.L_max * 2;
    double *lm_info = S.lm_info + (size_t)inst * S.L_max * 3;
    double *lm_tr = S.lm_tr + (size_t)inst * S.L_max;
    const int sh7 = 4 * L <= kThreads / 2 ? 2 : 2 * L <= kThreads / 2 ? 1 : 0, S7 = 1 << sh7;
    for (int j0 = 0; j0 < L; j0 += kThreads >> sh7) {
      const int j = j0 + (tid >> sh7), s7 = tid & (S7 - 1);
      const bool lwork = j < L;
      double v[6] = {0, 0, 0, 0, 0, 0};  // c00 c01 c10 c11 dx dy
      if (lwork) {
        for (int t = lstart[j] + s7; t < lstart[j + 1]; t += S7) {
          const int mq = lfac[t], p = mp[mq];
          const double *g = rec + (size_t)REC * mq;
          v[0] += g[6]; v[1] += g[7]; v[2] += g[8]; v[3] += g[9];
          const double dp0 = A[AT(np, 3 * p)], dp1 = A[AT(np, 3 * p + 1)], dp2 = A[AT(np, 3 * p + 2)];
          v[4] -= g[0] * dp0 + g[2] * dp1 + g[4] * dp2;
          v[5] -= g[1] * dp0 + g[3] * dp1 + g[5] * dp2;
        }
      }
      quad_butterfly(S7, v);
      if (!lwork || s7 != 0) continue;
      const double *lb = lamb + 8 * j;
      const double c00 = v[0] + lb[3], c01 = v[1] + lb[4], c10 = v[2] + lb[4], c11 = v[3] + lb[5];
      // delta_j = Lambda^-1 eta_j - sum_m G_m^T delta_p
      const double dx = v[4] + (lb[3] * lb[6] + lb[4] * lb[7]);
      const double dy = v[5] + (lb[4] * lb[6] + lb[5] * lb[7]);
      d_lm[2 * j] = dx;
      d_lm[2 * j + 1] = dy;
      est_lm[2 * j] = thl[2 * j] + dx;
      est_lm[2 * j + 1] = thl[2 * j + 1] + dy;
      if (hand) {
        thl[2 * j] = thl[2 * j] + dx;
        thl[2 * j + 1] = thl[2 * j + 1] + dy;
      }
      if (!full) continue;
      const double cs = 0.5 * (c01 + c10);
      lm_tr[j] = c00 + c11;
      const double id = 1.0 / (c00 * c11 - cs * cs);  // marginalCovariance(l).inverse() (SLAM2D.cpp:417)
      lm_info[3 * j] = c11 * id;
      lm_info[3 * j + 1] = -cs * id;
      lm_info[3 * j + 2] = c00 * id;
    }
  }
  // 7. pose estimates, information = inverse(covariance) by LLT (SLAM2D.cpp:395-408).  hand: LDS that receives est_pose [P][4]
  //    and, behind it at hand + 4 hand_cap, pose_info [P][6]
  __device__ __forceinline__ void pose_outputs(const DrlgxState &S, int tid, bool full, double *hand, int hand_cap) const {
    double *est_pose = S.est_pose + (size_t)inst * S.P_max * 4;
    double *pose_info = S.pose_info + (size_t)inst * S.P_max * 6;
    double *pose_tr = S.pose_tr + (size_t)inst * S.P_max;
    for (int i = (tid + kThreads / 2) % kThreads; i < P; i += kThreads) {
      const int k0 = 3 * i;
      const Pose t{thp[4 * i], thp[4 * i + 1], thp[4 * i + 2], thp[4 * i + 3]};
      const Pose e = compose(t, make_pose(A[AT(np, k0)], A[AT(np, k0 + 1)], A[AT(np, k0 + 2)]));
      est_pose[4 * i] = e.x; est_pose[4 * i + 1] = e.y; est_pose[4 * i + 2] = e.c; est_pose[4 * i + 3] = e.s;
      if (hand) {
        hand[4 * i] = e.x; hand[4 * i + 1] = e.y; hand[4 * i + 2] = e.c; hand[4 * i + 3] = e.s;
      }
      if (!full) continue;
      double c[6], info[6];  // c00 c10 c11 c20 c21 c22
      sigma_block(i, c);
      pose_tr[i] = c[0] + c[2] + c[5];
      inv3_sym_fast(c[0], c[1], c[3], c[2], c[4], c[5], info);
      for (int k = 0; k < 6; ++k) pose_info[6 * i + k] = info[k];
      if (hand)
        for (int k = 0; k < 6; ++k) hand[4 * hand_cap + 6 * i + k] = info[k];
    }
  }
  __device__ __forceinline__ void counters(const DrlgxState &S, int tid, bool refresh) const {
    if (tid != 0) return;
    int *cnt = S.cnt + (size_t)inst * DRLGX_CNT_STRIDE;
    if (!refresh) {
      cnt[C_ISAM] = count;
      cnt[C_NEWP] = P;
      cnt[C_NEWL] = L;
    }
    if (numeric_flag()) atomicMin(S.status, DRLGX_E_NUMERIC);
  }

  // everything after the simulator: all kThreads threads, hardware barriers.  Lfin / Mfin: the final counts (>= the front's).
  // hand: LDS (or null) that receives what the map stage of k_step reads next - est_pose [P][4] and, behind it at
  // hand + 4 hand_cap, pose_info [P][6] - so that it does not fetch them back from HBM; the landmark estimates are left in
  // `thl` for the same reason (the linearisation points are dead by then).  hand_cap: the pose capacity of those tables (the
  // launch's pose bound, LaunchSel::cap)
  template <int FT>
  __device__ __forceinline__ void back(const DrlgxState &S, int tid, int Lfin, int Mfin, bool full, bool refresh, double *hand = nullptr,
                                       const SimBox &box = SimBox{nullptr, nullptr, nullptr}, int hand_cap = 0) {
    const int L0 = L, M0 = M;
    L = Lfin; M = Mfin;
    append_step(S, tid, L0, box);
    __syncthreads();
    factor_tables(S, M0, M, tid, kThreads, box);
    __syncthreads();
    DRLGX_PROF(S, 1);
    close_landmarks(S, tid, M0);
    __syncthreads();
    DRLGX_PROF(S, 2);
    eliminate_landmarks(S, tid);
    __syncthreads();
    DRLGX_PROF(S, 3);
    const bool pre_e0 = Tn < FT;
    const v4d e0 = schur<FT>(S, tid, pre_e0);
    __syncthreads();
    DRLGX_PROF(S, 4);
    // 5. sweep: one tile row per wave; with nine / ten tile rows two light rows share a wave (k_sweep.hip)
    sweep_packed_fast<FT>(S, A, np, N, Tn, bad, tid, pre_e0, e0);
    __syncthreads();
    DRLGX_PROF(S, 5);
    double *d_pose = S.d_pose + (size_t)inst * S.P_max * 3;
    for (int k = tid; k < np; k += kThreads) d_pose[k] = A[AT(np, k)];
    if (full) landmark_marginals(tid);
    __syncthreads();
    DRLGX_PROF(S, 6);
    landmark_outputs(S, tid, full, hand != nullptr);
    pose_outputs(S, tid, full, hand, hand_cap);
    DRLGX_PROF(S, 7);
    counters(S, tid, refresh);
  }
};

// (contraction decided in the front end, like the incremental update that continues from this panel: k_inc.hip)
#pragma clang fp contract(on)
// The panel after a full (dense) solve: Sigma[:, active] from what SlamCtx::back leaves in LDS - A = -Sigma_pp (packed lower
// triangle), the per-factor G_m = Lambda_pl Lambda_ll^-1 blocks, the per-landmark factor lists:
//     Sigma_pl = -Sigma_pp G          (column block of landmark j: the sum over its factor list)
//     Sigma_ll = Lambda_ll^-1 + G^T Sigma_pp G = Lambda_ll^-1 - G^T Sigma_pl
// written to the HBM panel (the second stage reads the first one's rows back through L2).
struct __attribute__((aligned(8))) PanelPair {  // two adjacent panel entries (the landmark columns start at column 3: 8-byte aligned only)
  double x, y;
};
struct DensePanel {
  const SlamCtx &c;
  double *gpan, *jd;  // the instance's panel and its per-pose marginal blocks
  int ldg, P_max, P, L, pn;

  __device__ __forceinline__ double *prow(int q) const { return gpan + (size_t)q * ldg; }                // pose rows
  __device__ __forceinline__ double *lrow(int q) const { return gpan + (size_t)(3 * P_max + q) * ldg; }  // landmark rows
  __device__ __forceinline__ double asym(int i, int j) const { return c.A[c.AT(max(i, j), min(i, j))]; }
  // The work items of sigma_pl and sigma_ll are handed out through an LDS counter (SlamCtx::work_counter): list lengths are very
  // uneven - landmarks near the start are seen from most poses - and a static deal left some waves with twice the work of others.
  // One item per wave and call: false when all `limit` are taken
  __device__ __forceinline__ bool next_item(int *counter, int limit, int lane, int &w) const {
    w = 0;
    if (lane == 0) w = atomicAdd(counter, 1);
    w = __builtin_amdgcn_readfirstlane(w);
    return w < limit;
  }
  // pose rows: columns of the current pose, the marginal blocks
  __device__ __forceinline__ void pose_rows(int tid) const {
    for (int e = tid; e < 3 * P * 3; e += kThreads) {
      const int q = e / 3, cc = e - 3 * q;
      prow(q)[cc] = -asym(q, 3 * pn + cc);
    }
    for (int e = tid; e < 6 * P; e += kThreads) {
      const int i = e / 6, t = e - 6 * i;
      jd[e] = -c.A[c.sym3_index(i, t)];
    }
  }
  // Sigma_pl: one work item = (landmark j, pose i); the lanes of a wave share j and take consecutive poses, so that the walk over
  // j's factor list is uniform (one trip count, the G block and the observing pose are wave-uniform loads: no divergence - with
  // consecutive LANDMARKS per lane every wave paid for the longest list, ~40 entries against ~13 on average, and this stage plus
  // the next cost more than the whole dense solve: 74 us at 40 poses).  Same sums in the same order per output as before.
  // (Requesting the next factor's list entry, pose and G block under the current one's products - a hand-made two-stage pipeline of
  // the four dependent LDS round trips per factor - measured SLOWER: 17.9 -> 21.9 us at 40 poses, 20.6 -> 24.5 at 50.)
  __device__ __forceinline__ void sigma_pl(int tid) const {
    const int lane = tid & 63, ib = (P + 63) >> 6;  // pose blocks of 64 per landmark
    int w;
    while (next_item(c.work_counter(), L * ib, lane, w)) {
      const int j = w / ib, i = (w - j * ib) * 64 + lane;
      if (i >= P) continue;
      int rb[3];  // packed row starts of this pose's three rows
#pragma unroll
      for (int r = 0; r < 3; ++r) rb[r] = ((3 * i + r) * (3 * i + r + 1)) >> 1;
      double b[6] = {0, 0, 0, 0, 0, 0};
      const int t1 = c.lstart[j + 1];
      for (int t = c.lstart[j]; t < t1; ++t) {
        const int m = c.lfac[t], p = c.mp[m];
        const double *g = c.rec + (size_t)REC * m;
        const double g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3], g4 = g[4], g5 = g[5];
        const int c0 = 3 * p, cb0 = (c0 * (c0 + 1)) >> 1, cb1 = cb0 + c0 + 1, cb2 = cb1 + c0 + 2;  // (wave-uniform)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const int q = 3 * i + r;
          // asym(q, c) = A[max (max + 1) / 2 + min]
          const double a0 = c.A[q >= c0 ? rb[r] + c0 : cb0 + q], a1 = c.A[q >= c0 + 1 ? rb[r] + c0 + 1 : cb1 + q],
                       a2 = c.A[q >= c0 + 2 ? rb[r] + c0 + 2 : cb2 + q];
          b[2 * r] += a0 * g0 + a1 * g2 + a2 * g4;
          b[2 * r + 1] += a0 * g1 + a1 * g3 + a2 * g5;
        }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) *reinterpret_cast<PanelPair *>(prow(3 * i + r) + 3 + 2 * j) = PanelPair{b[2 * r], b[2 * r + 1]};
    }
  }
  // landmark rows: the columns of the current pose
  __device__ __forceinline__ void landmark_rows(int tid) const {
    for (int e = tid; e < 2 * L * 3; e += kThreads) {
      const int q = e / 3, cc = e - 3 * q;
      lrow(q)[cc] = prow(3 * pn + cc)[3 + q];
    }
  }
  // Sigma_ll: one work item = (landmark j, landmark j2), the lanes of a wave share j (uniform list walk, uniform G) and take
  // consecutive j2: the rows of Sigma_pl come back from L2 as contiguous 16-byte pieces
  __device__ __forceinline__ void sigma_ll(int tid) const {
    const int lane = tid & 63, jb = (L + 63) >> 6;
    int w;
    while (next_item(c.work_counter(), L * jb, lane, w)) {
      const int j = w / jb, j2 = (w - j * jb) * 64 + lane;
      if (j2 >= L) continue;
      double s00 = 0, s01 = 0, s10 = 0, s11 = 0;
      if (j == j2) {
        const double *lb = c.lamb + 8 * j;
        s00 = lb[3]; s01 = lb[4]; s10 = lb[4]; s11 = lb[5];
      }
      // (the rows come back through L2, ~1 us per dependent round trip: four list entries' loads are in flight together - the
      // longest list, ~40 entries, used to set this stage's time at one round trip per entry)
      const int t1 = c.lstart[j + 1];
      for (int t = c.lstart[j]; t < t1; t += 4) {
        const double *g[4];
        PanelPair x[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int m = c.lfac[min(t + u, t1 - 1)], p = c.mp[m];
          g[u] = c.rec + (size_t)REC * m;
#pragma unroll
          for (int kk = 0; kk < 3; ++kk) x[u][kk] = *reinterpret_cast<const PanelPair *>(prow(3 * p + kk) + 3 + 2 * j2);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (t + u >= t1) break;
#pragma unroll
          for (int kk = 0; kk < 3; ++kk) {
            const double x0 = x[u][kk].x, x1 = x[u][kk].y;
            s00 -= g[u][2 * kk] * x0; s01 -= g[u][2 * kk] * x1;
            s10 -= g[u][2 * kk + 1] * x0; s11 -= g[u][2 * kk + 1] * x1;
          }
        }
      }
      *reinterpret_cast<PanelPair *>(lrow(2 * j) + 3 + 2 * j2) = PanelPair{s00, s01};
      *reinterpret_cast<PanelPair *>(lrow(2 * j + 1) + 3 + 2 * j2) = PanelPair{s10, s11};
    }
  }
  // the panel's header: valid, for these counts
  __device__ __forceinline__ void publish(const DrlgxState &S, int tid) const {
    if (tid != 0) return;
    int *meta = inc_meta(S, c.inst);
    meta[0] = 1; meta[1] = P; meta[2] = L; meta[3] = c.M;
    if (S.inc_stats) atomicAdd(S.inc_stats + 1, 1ull);
  }
};
__device__ __forceinline__ void panel_from_dense(const DrlgxState &S, const SlamCtx &c, int tid) {
  if (!S.jc) return;
  const DensePanel d{c, S.jc + (size_t)c.inst * S.jc_stride, S.jd + (size_t)c.inst * S.P_max * 6, S.jc_ld, S.P_max, c.P, c.L, c.P - 1};
  DRLGX_PROF(S, 44);
  if (tid == 0) *c.work_counter() = 0;
  d.pose_rows(tid);
  __syncthreads();
  d.sigma_pl(tid);
  __syncthreads();
  DRLGX_PROF(S, 45);
  if (tid == 0) *c.work_counter() = 0;
  d.landmark_rows(tid);
  __syncthreads();
  d.sigma_ll(tid);
  DRLGX_PROF(S, 46);
  d.publish(S, tid);
}

#pragma clang fp contract(fast)
// The SLAM stage after the simulator.  `pre` (have_pre): the context whose front() already ran beside the simulator (k_step)
// for the counts before the step (records in LDS).  smem_off: first byte of the dynamic LDS the stage may use.
template <int FT>
__device__ __forceinline__ void slam_finish(const DrlgxState &S, const LaunchSel &sel, int lds_bytes, size_t smem_off, const SlamCtx &pre, bool have_pre,
                                            const int *mail = nullptr, double *hand = nullptr, const double **lm_out = nullptr,
                                            SimBox box = SimBox{nullptr, nullptr, nullptr}, int hand_cap = 0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = drlgx_tid();
  const int bi = drlgx_bid();
  if (!sel.on(bi)) return;
  const int inst = sel.base + bi;
  int *cnt = S.cnt + (size_t)inst * DRLGX_CNT_STRIDE;
  // `full`: the block marginals are wanted.  Look-ahead rollouts only need them at their last action (the virtual map is
  // rebuilt there and nowhere else): the steps before it solve for the estimates only.  If that last action was rejected
  // (nothing was appended) the marginals of the unchanged system are recomputed without counting as an update.
  const bool full = sel.map_on(bi);
  // (mail: the counts after the step as the simulator wave left them in LDS - no round trip to HBM; -1: it appended nothing)
  const bool mailed = mail && mail[0] >= 0;
  const bool refresh = mailed ? false : cnt[C_FLAG] != 0;
  if (refresh && !(sel.map_last_only && sel.n_act && full)) return;
  const int P = mailed ? mail[0] : cnt[C_P], L = mailed ? mail[1] : cnt[C_L], M = mailed ? mail[2] : cnt[C_M];
  if ((3 * P + 1 + 15) / 16 > kDenseTiles) {
    // more poses than this kernel was launched for (the host's bound was wrong): flag it, touch nothing
    if (tid == 0) atomicMin(S.status, DRLGX_E_CAPACITY);
    return;
  }
  DRLGX_PROF(S, 0);
  SlamCtx c;
  const bool from_pre = have_pre && !refresh && pre.P == P && L <= pre.Lb && M <= pre.Mb;
  if (from_pre) {
    c = pre;
  } else {
    // stand-alone kernel, a rejected move, or more new landmarks / factors than the front reserved room for: everything now
    const int n_old_p = cnt[C_NEWP], n_old_l = cnt[C_NEWL], count = cnt[C_ISAM] + (refresh ? 0 : 1);
    if (SlamCtx::big_fits(smem_off, lds_bytes, P, L, M)) c.setup<true>(S, smem_raw, smem_off, lds_bytes, inst, P, L, M);
    else c.setup<false>(S, smem_raw, smem_off, lds_bytes, inst, P, L, M);
    c.front<false>(S, tid, P, L, M, n_old_p, n_old_l, count, refresh, nullptr, SubBarrier{nullptr, 0, 0});
    __syncthreads();
  }
  c.back<FT>(S, tid, L, M, full, refresh, hand, (from_pre && mailed) ? box : SimBox{nullptr, nullptr, nullptr}, hand_cap);
  if (lm_out) *lm_out = c.lm_estimates();
  if (S.jc && !refresh) {  // the covariance panel the incremental updates continue from (k_inc.hip)
    __syncthreads();
    panel_from_dense(S, c, tid);
  }
}

template <int FT>
__device__ __forceinline__ void slam_body(const DrlgxState &S, const LaunchSel &sel, int lds_bytes) {
  if (inc_stage<0>(S, sel, lds_bytes, 0)) return;
  SlamCtx none;
  slam_finish<FT>(S, sel, lds_bytes, 0, none, false);
}

template <int FT>
__global__ __launch_bounds__(kThreads) void k_slam(DRLGX_KS_PARAM, LaunchSel sel, int lds_bytes) {
  const DrlgxState &S = DRLGX_KS_REF;
  slam_body<FT>(S, sel, lds_bytes);
}
#pragma clang fp contract(off)
}  // namespace kslam
