// Block Gauss-Jordan sweep primitives on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), shared by every SLAM solver of
// the unity build k_step.hip: the dense solver (k_slam.hip), the incremental update (k_inc.hip) and the pose-chain solver
// (k_slam_arrow.hip; its workspace sweep, k_sweep_ws.hip, builds on the helpers here).
//   mfma4 / ld4 / ks16, readlane_f64, row_bcast_lane, rowgroup_bcast, the dpp_* helpers   operand and lane plumbing
//   fast_rcp, inv16_blk      in-wave inversion of a 16 x 16 SPD tile by 4 x 4 block pivots
//   SweepRow, sweep_role     one tile row of the sweep in accumulator registers; the block-step loop of one wave
//   sweep_packed_fast        the sweep of a packed system of up to ten tile rows held in LDS (all 512 threads)
#pragma once
#include "drlgx_dev.h"
namespace kslam {
#pragma clang fp contract(fast)  // (the unity build k_step.hip is compiled with -ffp-contract=off)
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
typedef double v4d __attribute__((ext_vector_type(4)));
// doubles of the LDS region of a packed N x N system swept by sweep_packed_fast: the packed lower triangle, or the sweep's
// panels (two pivot-column panels, two W panels, two E tiles, two diagonal-tile dumps) that alias it
// (+ 6 N + 64 behind the triangle: SlamCtx::front parks 18 doubles per pose there - up to N = 128 the panels' size covers it)
__host__ __device__ constexpr size_t sweep_region_doubles(size_t N) {
  const size_t a = N * (N + 1) / 2 + 6 * N + 64, b = 64 * N + 1024;
  return a > b ? a : b;
}

// (fast_rcp and inv16_blk are shared with the incremental update (k_inc.hip), whose fused and staged forms must round alike
// although they are inlined into differently shaped code: contraction decided in the front end for them)
#pragma clang fp contract(on)
// 1/x to double round-off: v_rcp_f64 + two Newton steps (the pivot inverse is on every thread's critical path)
__device__ __forceinline__ double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = r * (2.0 - x * r);
  r = r * (2.0 - x * r);
  return r;
}

#pragma clang fp contract(fast)
struct SweepCtx {
  int I, lane, lc, lr, np, N;
  bool live;   // this wave's tile row holds real rows (I < number of 16-row blocks in use)
  bool ewave;  // this wave inverts the diagonal tiles (an idle tile row if there is one, else tile row 0)
  int *bad;
  long long *tr;  // dev aid: 5 cycle stamps per wave for one step (armed through drlgx_debug_phase_clocks_host)
};

// ------------------------------------------------------------------------------------------------------------------
// 16-wide block Gauss-Jordan on lower tiles in MFMA accumulators (diagonal tiles kept fully symmetric).  Scalar branches
// cost ~20-30 cycles here and a block barrier ~50 plus the arrival skew, so a step pivots on a whole 16 x 16 tile column K
// (7 steps at 37 poses):
//   P  the pivot tile column is published to LDS: panel PAN[i][.] = A[i][16 K + .]
//   W  every wave: W_I = PAN_I E_K  (4 chained MFMAs, E_K = -D_K^-1 from the look-ahead below)
//   U  every wave: A_Iu += W_I PAN_u^T for its tiles u <= I (4 MFMAs each); tile column K <- -W_I; pivot rows <- -W_u^T,
//      pivot block <- E_K
//   look-ahead: the diagonal tile D_{K+1} = A_{K+1,K+1} + W_{K+1} PAN_{K+1}^T is formed and inverted inside ONE wave with
//      little or no matrix work while the others run U.
// sweep_role (below) keeps the panels as MFMA operand images and needs one barrier per step.  ks16 / ld4 serve the row-major
// "KS" layout: a 16-vector v is stored as v[(c & 3) * 4 + (c >> 2)], so that the 4 K-steps of an MFMA operand lane are one
// 32-byte read (the Y / U' / W' images of k_inc.hip, the panels of k_sweep_ws.hip).
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ks16(int c) { return (c & 3) * 4 + (c >> 2); }

__device__ __forceinline__ v4d mfma4(const double (&a)[4], const double (&b)[4], v4d c) {
#pragma unroll
  for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], c, 0, 0, 0);
  return c;
}
__device__ __forceinline__ void ld4(const double *p, double (&o)[4]) {
  const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
  o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
}

__device__ __forceinline__ double readlane_f64(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, src), hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// ---- lane broadcasts without LDS: DPP row broadcasts and the gfx950 permlane swaps ----
template <int kLane>
__device__ __forceinline__ double row_bcast_lane(double v) {  // value of lane kLane of each 16-lane row
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp((int)b, (int)b, 0x150 + kLane, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp((int)(b >> 32), (int)(b >> 32), 0x150 + kLane, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int kRow>
__device__ __forceinline__ double rowgroup_bcast(double v) {  // 16-lane row kRow (0..3) copied to all four rows
  const long long b = __double_as_longlong(v);
  unsigned w[2] = {(unsigned)b, (unsigned)(b >> 32)};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const auto p16 = __builtin_amdgcn_permlane16_swap(w[h], w[h], false, false);  // [x0 x0 x2 x2], [x1 x1 x3 x3]
    const unsigned y = (kRow & 1) ? p16[1] : p16[0];
    const auto p32 = __builtin_amdgcn_permlane32_swap(y, y, false, false);        // [A A A A], [B B B B]
    w[h] = (kRow & 2) ? p32[1] : p32[0];
  }
  return __longlong_as_double(((long long)w[1] << 32) | w[0]);
}

#pragma clang fp contract(on)
// ---- in-wave 16 x 16 SPD inversion by 4 x 4 BLOCK pivots on the fp64 matrix cores ----
// Same contract as the scalar-pivot inv16 of k_sweep_ws.hip (d: full symmetric tile in accumulator layout <- -D^-1 on the
// first `nact` pivots), four block steps instead of sixteen scalar ones.  Block step Kb (rows / columns 4 Kb .. 4 Kb + 3 = accumulator register Kb):
//   E4 = -(pivot block)^-1                  closed form (2 x 2 blocks, two reciprocals), from ten v_readlane values
//   W^T = E4 D[Kb rows, :]                  ONE MFMA: A operand = E4 (lanes lc < 4), B operand = register Kb as it is;
//                                           output register 0 at lane (lr, lc) = W[lc][lr] = the A operand of the update
//   D <- D + W (D[Kb rows, :] with the pivot columns replaced by -I)   ONE MFMA; with the pivot columns of the
//                                           accumulator input zeroed this leaves -W there, exactly
//   pivot rows <- -W^T, pivot block <- E4   selects
// The dependent chain per block is ~25 fp64 operations + two MFMAs instead of four scalar pivots of ~10 operations plus
// their permlane / DPP broadcasts (scripts/emul/inv16_blk_emul.py checks the index algebra against numpy).
struct Inv16Lane {  // lane constants of the block inversion
  bool lr1, c1, top, left, ua, ub, lc_lt4;
  double sel;  // -1 where (lc & 3) == lr, else 0: the "-I" of the pivot columns in the B operand
  __device__ __forceinline__ Inv16Lane(int lr, int lc) {
    lr1 = lr & 1; c1 = lc & 1; top = lr < 2; left = (lc & 3) < 2;
    ua = top ? c1 : lr1; ub = top ? lr1 : c1;
    lc_lt4 = lc < 4;
    sel = ((lc & 3) == lr) ? -1.0 : 0.0;
  }
};
template <int Kb>
__device__ __forceinline__ void inv16_blk_step(const SweepCtx &x, const Inv16Lane &q, v4d &d, bool &spd) {
  constexpr int c0 = 4 * Kb;
  const double a00 = readlane_f64(d[Kb], c0);
  const double a10 = readlane_f64(d[Kb], 16 + c0), a11 = readlane_f64(d[Kb], 16 + c0 + 1);
  const double a20 = readlane_f64(d[Kb], 32 + c0), a21 = readlane_f64(d[Kb], 32 + c0 + 1), a22 = readlane_f64(d[Kb], 32 + c0 + 2);
  const double a30 = readlane_f64(d[Kb], 48 + c0), a31 = readlane_f64(d[Kb], 48 + c0 + 1), a32 = readlane_f64(d[Kb], 48 + c0 + 2),
               a33 = readlane_f64(d[Kb], 48 + c0 + 3);
  // P = [a00 a10; a10 a11], Q = [a20 a21; a30 a31], R = [a22 a32; a32 a33]: block inverse through S = R - Q P^-1 Q^T.
  // (A variant that carries det P as a scale, so that the two reciprocals are not in sequence - dependent depth ~16
  // instead of ~29 operations - measured SLOWER, 3172 against 2988 cycles per tile: the step is bound by instruction
  // issue of the one wave that runs it, not by latency; scripts/micro/inv16_bench.hip.)
  const double detp = a00 * a11 - a10 * a10;
  const double ip = fast_rcp(detp);
  const double p00 = a11 * ip, p10 = -a10 * ip, p11 = a00 * ip;           // P^-1
  const double t00 = a20 * p00 + a21 * p10, t01 = a20 * p10 + a21 * p11;  // T = Q P^-1
  const double t10 = a30 * p00 + a31 * p10, t11 = a30 * p10 + a31 * p11;
  const double s00 = a22 - (t00 * a20 + t01 * a21);                       // S = R - T Q^T
  const double s10 = a32 - (t10 * a20 + t11 * a21);
  const double s11 = a33 - (t10 * a30 + t11 * a31);
  const double dets = s00 * s11 - s10 * s10;
  const double is = fast_rcp(dets);
  const double r00 = s11 * is, r10 = -s10 * is, r11 = s00 * is;           // S^-1
  const double u00 = r00 * t00 + r10 * t10, u01 = r00 * t01 + r10 * t11;  // U = S^-1 T
  const double u10 = r10 * t00 + r11 * t10, u11 = r10 * t01 + r11 * t11;
  spd = spd && (a00 > 0) && (detp > 0) && (s00 > 0) && (dets > 0);  // (tested once per tile: off the dependent chain)
  // this lane's entry E4[lr][lc & 3] of  E4 = -D^-1 = -[P^-1 + T^T U, -U^T; -U, S^-1]
  const double t0x = q.lr1 ? t01 : t00, t1x = q.lr1 ? t11 : t10;  // T[.][lr & 1]
  const double u0c = q.c1 ? u01 : u00, u1c = q.c1 ? u11 : u10;    // U[.][lc & 1]
  const double pI = (q.lr1 == q.c1) ? (q.lr1 ? p11 : p00) : p10;
  const double rI = (q.lr1 == q.c1) ? (q.lr1 ? r11 : r00) : r10;
  const double e_tl = -(pI + t0x * u0c + t1x * u1c);
  const double uo = q.ua ? (q.ub ? u11 : u10) : (q.ub ? u01 : u00);  // U[lr - 2][c] below the diagonal, U[c - 2][lr] above
  const double e_lane = (q.top == q.left) ? (q.top ? e_tl : -rI) : uo;
  const double eA = q.lc_lt4 ? e_lane : 0.0;
  const v4d z = {0.0, 0.0, 0.0, 0.0};
  const v4d wt4 = __builtin_amdgcn_mfma_f64_16x16x4f64(eA, d[Kb], z, 0, 0, 0);
  const double wt = wt4[0];  // lane (lr, lc): W[lc][lr],  W = D[:, Kb columns] E4
  const bool inK = (x.lc >> 2) == Kb;
  const double bop = inK ? q.sel : d[Kb];
  v4d cin;
#pragma unroll
  for (int r = 0; r < 4; ++r) cin[r] = inK ? 0.0 : d[r];
  d = __builtin_amdgcn_mfma_f64_16x16x4f64(wt, bop, cin, 0, 0, 0);
  d[Kb] = inK ? e_lane : -wt;
}
// nact: number of pivots of this tile (1 .. 16); the rows / columns beyond are not pivots and their content afterwards is
// finite but meaningless (every user of E multiplies them by the zeroed panel columns or never reads them)
// kSkip: block steps whose four pivots are all inactive are left out (the incremental update's k x k systems, k <= 16: the
// inactive part is an identity block, decoupled from the rest)
template <bool kSkip = false>
__device__ __forceinline__ void inv16_blk(const SweepCtx &x, int nact, v4d &d) {
  if (nact < 16) {  // decouple the inactive rows / columns: identity there
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = x.lr + 4 * r;
      if (row >= nact || x.lc >= nact) d[r] = (row == x.lc) ? 1.0 : 0.0;
    }
  }
  const Inv16Lane q(x.lr, x.lc);
  bool spd = true;
  inv16_blk_step<0>(x, q, d, spd);
  if (!kSkip || nact > 4) inv16_blk_step<1>(x, q, d, spd);
  if (!kSkip || nact > 8) inv16_blk_step<2>(x, q, d, spd);
  if (!kSkip || nact > 12) inv16_blk_step<3>(x, q, d, spd);
  if (!spd && x.lane == 0) x.bad[0] = 1;
}

#pragma clang fp contract(fast)
// ---- the sweep of a packed system as ONE runtime loop over the block steps ----
// (A block step instantiated per tile column is 145 KB of straight-line code for seven steps - more than twice the 64 KB
// instruction cache, so the wave that inverts the diagonal tiles, alone on the critical path, would run out of cold
// instruction fetches: 5.3 k cycles against 3.8 k warm.)  One copy of the step serves every tile column K; the accumulator
// tile "K" is selected by uniform branches over the statically indexed registers.
//
// LDS panels are stored as OPERAND IMAGES: a 16 x 16 block X is kept as the four MFMA operand registers of every lane,
//   img[(s >> 1) * 128 + 2 * lane + (s & 1)] = X[lc][4 s + lr],
// two lane-linear 16-byte halves (conflict-free ds_read_b128 / ds_write_b128; a row-major [16] KS layout puts every lane of
// a 16-lane group on two banks).  The same registers serve as the A operand of X . and as the B operand of
// . X^T.  With that, products are formed TRANSPOSED so that an MFMA result is directly the next MFMA's operand:
//   W_I^T = E_K PAN_I^T   (A = image of E_K (symmetric), B = image of PAN_I)   -> registers = image of W_I
//   A_Iu += W_I PAN_u^T   (A = those registers, B = image of PAN_u)
// and the E-wave's look-ahead  D_{K+1} += W_{K+1} PAN_{K+1}^T needs no LDS round trip.  A wave needs the W of
// other waves only for the pivot rows (A_Ku <- -W_u^T); that replacement is deferred until after the next step's barrier
// (W images double buffered), which leaves ONE workgroup barrier per block step instead of two.
struct SwL {  // every buffer twice (index = block step & 1); address arithmetic, no pointer tables (they would go to scratch)
  double *base;  // pan[2][16 N] operand images of the pivot tile column, wt[2][16 N] images of W_I = PAN_I E_K,
  int n16;       // einv[2][256] image of E_K = -D_K^-1 (= the accumulator registers of the inverting wave),
                 // dscr[2][256] accumulator registers of the next diagonal tile (lane-linear)
  __device__ __forceinline__ double *pan(int b) const { return base + b * n16; }
  __device__ __forceinline__ double *wt(int b) const { return base + (2 + b) * n16; }
  __device__ __forceinline__ double *einv(int b) const { return base + 4 * n16 + b * 256; }
  __device__ __forceinline__ double *dscr(int b) const { return base + 4 * n16 + 512 + b * 256; }
};
__device__ __forceinline__ void ld_op(const double *img, int lane, double (&o)[4]) {
  const double2 a = *reinterpret_cast<const double2 *>(img + 2 * lane), b = *reinterpret_cast<const double2 *>(img + 128 + 2 * lane);
  o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
}
__device__ __forceinline__ void st_op(double *img, int lane, double v0, double v1, double v2, double v3) {
  *reinterpret_cast<double2 *>(img + 2 * lane) = make_double2(v0, v1);
  *reinterpret_cast<double2 *>(img + 128 + 2 * lane) = make_double2(v2, v3);
}
// offset inside an operand image of the element (row lr + 4 r, column lc) that a lane holds in accumulator layout
__device__ __forceinline__ int acc_off(int lr, int lc, int r) {
  return (lc >> 3) * 128 + 2 * (16 * (lc & 3) + lr + 4 * r) + ((lc >> 2) & 1);
}

// ONE TILE ROW of the sweep: the tiles (R, 0 .. R) in accumulator registers and what the block steps do to them.  R is a
// compile-time constant (R = -1: no row) - every register index except "tile column K" is static and the tile loops have no
// branches.  A role (below) owns one row or two.
template <int R>
struct SweepRow {
  static constexpr int NT = R >= 0 ? R + 1 : 1;
  v4d acc[NT];
  static __device__ __forceinline__ int AT(int i, int j) { return i * (i + 1) / 2 + j; }

  __device__ __forceinline__ void load(const double *A, int N, int lr, int lc) {
    if constexpr (R >= 0) {
#pragma unroll
      for (int u = 0; u <= R; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * R + lr + 4 * r, j = 16 * u + lc;
          acc[u][r] = (i < N && j < N) ? A[AT(max(i, j), min(i, j))] : 0.0;
        }
    }
  }
  // the first diagonal tile, for E_0
  __device__ __forceinline__ void dump_d0(const SwL &L, int lane) {
    if constexpr (R == 0) st_op(L.dscr(0), lane, acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
  }
  // ---- P: publish the pivot tile column (masked columns / rows as zeros) ----
  __device__ __forceinline__ void publish(const SwL &L, int K, int np, bool have_next, int lane, int lr, int lc, const int (&aoff)[4]) {
    if constexpr (R >= 0) {
      const int kb = 16 * K;
      double *pan = L.pan(K & 1);
      if (K <= R) {
        const bool colact = kb + lc < np;
        double *pI = pan + 256 * R;
#pragma unroll
        for (int u = 0; u <= R; ++u)  // (a ladder of scalar branches selects the statically indexed tile K)
          if (u == K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) pI[aoff[r]] = colact ? acc[u][r] : 0.0;
          }
        if (K == R) {  // the transposed tiles (R, u < R): accumulator registers = operand image of PAN_u
#pragma unroll
          for (int u = 0; u < R; ++u)
            st_op(pan + 256 * u, lane, (kb + lr < np) ? acc[u][0] : 0.0, (kb + lr + 4 < np) ? acc[u][1] : 0.0,
                  (kb + lr + 8 < np) ? acc[u][2] : 0.0, (kb + lr + 12 < np) ? acc[u][3] : 0.0);
        }
      }
      if (have_next && K + 1 == R)  // current values of the next diagonal tile, for the look-ahead
        st_op(L.dscr((K + 1) & 1), lane, acc[NT - 1][0], acc[NT - 1][1], acc[NT - 1][2], acc[NT - 1][3]);
    }
  }
  // ---- deferred from step K - 1: its pivot rows A_{K-1,u} <- -(W_u)^T (all rows active: only the last block is masked) ----
  __device__ __forceinline__ void deferred(const SwL &L, int K, int lane) {
    if constexpr (R >= 1) {
      if (K == R + 1) {
        const double *wp = L.wt((K - 1) & 1);
#pragma unroll
        for (int u = 0; u < R; ++u) {
          double t[4];
          ld_op(wp + 256 * u, lane, t);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[u][r] = -t[r];
        }
      }
    }
  }
  // ---- W, U ----
  __device__ __forceinline__ void update(const SwL &L, int K, int np, int lane, int lr, int lc, const int (&aoff)[4]) {
    if constexpr (R >= 0) {
      const int kb = 16 * K, b = K & 1;
      const bool has_mask = np < kb + 16;  // the last block holds the rhs row / pads: they are not pivots
      const double *pan = L.pan(b);
      double aP[4], eB[4];
      ld_op(pan + 256 * R, lane, aP);
      ld_op(L.einv(b), lane, eB);
      v4d wv = {0.0, 0.0, 0.0, 0.0};
      wv = mfma4(eB, aP, wv);  // image of W_R
      double *wI = L.wt(b) + 256 * R;
      st_op(wI, lane, wv[0], wv[1], wv[2], wv[3]);
      const double aW[4] = {wv[0], wv[1], wv[2], wv[3]};
      if (K != R || has_mask) {
        // A_Ru += W_R PAN_u^T (tile column K is replaced below, except in wave K whose masked rows keep the update); the
        // next tile's operand is loaded while this tile's MFMAs run
        // two tiles at a time: their MFMA chains are independent, so the matrix pipe is issued back to back (a chain on
        // ONE accumulator waits ~20 cycles per link for the previous result)
        double bP[2][2][4];
        ld_op(pan, lane, bP[0][0]);
        if (R >= 1) ld_op(pan + 256, lane, bP[0][1]);
#pragma unroll
        for (int u = 0; u <= R; u += 2) {
          constexpr int R1 = R >= 0 ? R : 0;
          const int h = (u >> 1) & 1, u1 = u + 1 <= R1 ? u + 1 : u;
          if (u + 2 <= R) ld_op(pan + 256 * (u + 2), lane, bP[h ^ 1][0]);
          if (u + 3 <= R) ld_op(pan + 256 * (u + 3), lane, bP[h ^ 1][1]);
          const bool d0 = u != K || K == R, d1 = u + 1 <= R && (u + 1 != K || K == R);
          if (d0 && d1) {
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
              acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(aW[s2], bP[h][0][s2], acc[u], 0, 0, 0);
              acc[u1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aW[s2], bP[h][1][s2], acc[u1], 0, 0, 0);
            }
          } else if (d0) {
            acc[u] = mfma4(aW, bP[h][0], acc[u]);
          } else if (d1) {
            acc[u1] = mfma4(aW, bP[h][1], acc[u1]);
          }
        }
      }
      if (K <= R) {
        wave_lds_sync();  // own image -> accumulator layout
        double w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = wI[aoff[r]];
        if (K < R) {
#pragma unroll
          for (int u = 0; u < R; ++u)
            if (u == K) {
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[u][r] = -w[r];  // A_RK <- A_RK D^-1 (masked columns: W = 0)
            }
        } else {
          // pivot block <- E_K; rows >= np (rhs, pads) keep the regular update, their pivot columns take -W like any other
          // row; the pivot rows of the tiles (K, u < K) follow after the next barrier
          const bool colact = kb + lc < np;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool rowact = kb + lr + 4 * r < np;
            acc[NT - 1][r] = rowact ? (colact ? eB[r] : -aW[r]) : (colact ? -w[r] : acc[NT - 1][r]);
          }
        }
      }
    }
  }
  // the pivot rows of the last block (masked: rows >= np keep their regular update)
  __device__ __forceinline__ void last_rows(const SwL &L, int nK, int np, int lane, int lr) {
    if constexpr (R >= 1) {
      if (R == nK - 1) {
        const int kb = 16 * R;
        const double *wp = L.wt(R & 1);
#pragma unroll
        for (int u = 0; u < R; ++u) {
          double t[4];
          ld_op(wp + 256 * u, lane, t);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[u][r] = (kb + lr + 4 * r < np) ? -t[r] : acc[u][r];
        }
      }
    }
  }
  __device__ __forceinline__ void store(double *A, int N, int lr, int lc) const {
    if constexpr (R >= 0) {
#pragma unroll
      for (int u = 0; u <= R; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * R + lr + 4 * r, j = 16 * u + lc;
          if (j <= i && i < N) A[AT(i, j)] = acc[u][r];
        }
    }
  }
};

// The sweep of ONE ROLE: the wave that owns tile row I (I = -1: none), a second one I2 (the nine- and ten-row systems of 43 .. 53
// poses: two light rows share a wave, so that every wave still runs ONE block-step loop with ONE barrier per step) and, with kE,
// inverts the diagonal tiles.  The block steps are a runtime loop, so each wave runs a few KB of code that stays in the
// instruction cache.
// A: the packed lower triangle (LDS); the panels alias it once the tiles are in registers.  Every role executes the same
// sequence of workgroup barriers.
// have_e0 (kE only): e0 = E_0 = -D_0^-1 as the caller inverted it already (SlamCtx::back does, under the Schur phase); by
// value - a pointer to it would put it into scratch memory
template <int I, bool kE, int I2 = -1>
__device__ __forceinline__ void sweep_role(const DrlgxState &S, const SweepCtx &x, double *A, int N, bool have_e0 = false,
                                           v4d e0 = v4d{0.0, 0.0, 0.0, 0.0}) {
  const int lane = x.lane, lc = x.lc, lr = x.lr, np = x.np;
  const int nK = (np + 15) >> 4;
  SweepRow<I> r1;
  SweepRow<I2> r2;
  r1.load(A, N, lr, lc);
  r2.load(A, N, lr, lc);
  __syncthreads();  // every tile is in registers: the LDS region of A now holds the sweep panels
  const SwL L{A, 16 * N};
  r1.dump_d0(L, lane);
  r2.dump_d0(L, lane);
  __syncthreads();
  if constexpr (kE) {  // E_0
    if (have_e0) {
      st_op(L.einv(0), lane, e0[0], e0[1], e0[2], e0[3]);
    } else {
      double t[4];
      ld_op(L.dscr(0), lane, t);
      v4d d = {t[0], t[1], t[2], t[3]};
      inv16_blk(x, min(16, np), d);
      st_op(L.einv(0), lane, d[0], d[1], d[2], d[3]);
    }
  }
  const int aoff[4] = {acc_off(lr, lc, 0), acc_off(lr, lc, 1), acc_off(lr, lc, 2), acc_off(lr, lc, 3)};
#pragma clang loop unroll(disable)
  for (int K = 0; K < nK; ++K) {
    const int kb = 16 * K, b = K & 1;
    const bool have_next = kb + 16 < np;
    const bool trg = x.tr && K == 3;
    if (trg) x.tr[0] = clock64();
    r1.publish(L, K, np, have_next, lane, lr, lc, aoff);
    r2.publish(L, K, np, have_next, lane, lr, lc, aoff);
    if (trg) x.tr[1] = clock64();
    __syncthreads();  // panels of step K, E_K, the W images of step K - 1
    const double *pan = L.pan(b);
    r1.deferred(L, K, lane);
    r2.deferred(L, K, lane);
    // ---- look-ahead (critical path): E_{K+1} = -(D_{K+1} + W_{K+1} PAN_{K+1}^T)^-1 ----
    if constexpr (kE) {
      if (have_next) {
        // (this chain is the critical path of the whole sweep: it outranks the SIMD partner's update work)
        __builtin_amdgcn_s_setprio(3);
        double aP[4], eB[4], t[4];
        ld_op(pan + 256 * (K + 1), lane, aP);
        ld_op(L.einv(b), lane, eB);
        ld_op(L.dscr((K + 1) & 1), lane, t);
        v4d w1 = {0.0, 0.0, 0.0, 0.0};
        w1 = mfma4(eB, aP, w1);  // image of W_{K+1}
        const double aW[4] = {w1[0], w1[1], w1[2], w1[3]};
        v4d dn = {t[0], t[1], t[2], t[3]};
        dn = mfma4(aW, aP, dn);
        if (trg) x.tr[2] = clock64();
        inv16_blk(x, min(16, np - kb - 16), dn);
        st_op(L.einv((K + 1) & 1), lane, dn[0], dn[1], dn[2], dn[3]);
        __builtin_amdgcn_s_setprio(0);
        if (trg) x.tr[3] = clock64();
      }
    }
    r1.update(L, K, np, lane, lr, lc, aoff);
    r2.update(L, K, np, lane, lr, lc, aoff);
    if (trg) x.tr[4] = clock64();
  }
  __syncthreads();
  r1.last_rows(L, nK, np, lane, lr);
  r2.last_rows(L, nK, np, lane, lr);
  __syncthreads();
  r1.store(A, N, lr, lc);
  r2.store(A, N, lr, lc);
}

// sum over the aligned groups of 8 lanes, in the lane with (lane & 7) == 7: DPP row shifts, no LDS traffic
template <int kCtrl>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, kCtrl, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), kCtrl, 0xf, 0xf, true);
  return v + __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// the value of another lane of the same quad: kCtrl = DPP quad_perm (0xB1: lane ^ 1, 0x4E: lane ^ 2)
template <int kCtrl>
__device__ __forceinline__ double dpp_quad_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, kCtrl, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), kCtrl, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double sum8_lane7(double v) {
  v = dpp_add_f64<0x111>(v);  // row_shr:1
  v = dpp_add_f64<0x112>(v);  // row_shr:2
  v = dpp_add_f64<0x114>(v);  // row_shr:4
  return v;
}

// Symmetric Gauss-Jordan sweep of the packed lower triangle `A` (LDS, row i at i (i + 1) / 2, N = 16 Tn <= 16 FT rows; the
// region must hold sweep_region_doubles(N) doubles: the sweep panels alias it while the tiles are in registers) on
// the pivots [0, np); rows >= np (the rhs row np, pads) are carried along.  Afterwards A holds -A_pp^-1 and row np the
// solution.  All kThreads threads of the workgroup call it (block barriers inside).
template <int FT>
__device__ __forceinline__ void sweep_packed_fast(const DrlgxState &S, double *A, int np, int N, int Tn, int *bad, int tid, bool have_e0 = false,
                                                  v4d e0 = v4d{0.0, 0.0, 0.0, 0.0}) {
  static_assert(FT == 8, "one role per wave of the 512-thread workgroup");
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (Tn > FT) {
    // Nine or ten tile rows (43 .. 53 poses): the wave of row 0 inverts the diagonal tiles, rows 1 + 2 share a wave (five tiles), with
    // ten rows 3 + 4 too (nine); waves w and w + 4 share a SIMD - light next to heavy:
    //   ten rows:  SIMD 0: {E, 0} + {9}   1: {1, 2} + {8}   2: {3, 4} + {5}   3: {6} + {7}      (11 / 14 / 15 / 15 tiles)
    //   nine rows: SIMD 0: {E, 0} + {8}   1: {1, 2} + {7}   2: {3} + {6}      3: {4} + {5}      (10 / 13 / 11 / 11)
    const SweepCtx x{0, lane, lane & 15, lane >> 4, np, N, true, wv == 0, bad,
                     (S.prof && blockIdx.x == S.prof_block && lane == 0) ? S.prof + 64 + 5 * wv : nullptr};
    const bool ten = Tn == 10;
    switch (wv) {
      case 0: sweep_role<0, true>(S, x, A, N); break;
      case 1: sweep_role<1, false, 2>(S, x, A, N); break;
      case 2:
        if (ten) sweep_role<3, false, 4>(S, x, A, N);
        else sweep_role<3, false>(S, x, A, N);
        break;
      case 3:
        if (ten) sweep_role<6, false>(S, x, A, N);
        else sweep_role<4, false>(S, x, A, N);
        break;
      case 4:
        if (ten) sweep_role<9, false>(S, x, A, N);
        else sweep_role<8, false>(S, x, A, N);
        break;
      case 5:
        if (ten) sweep_role<8, false>(S, x, A, N);
        else sweep_role<7, false>(S, x, A, N);
        break;
      case 6:
        if (ten) sweep_role<5, false>(S, x, A, N);
        else sweep_role<6, false>(S, x, A, N);
        break;
      default:
        if (ten) sweep_role<7, false>(S, x, A, N);
        else sweep_role<5, false>(S, x, A, N);
        break;
    }
    return;
  }
  // tile rows r and FT-1-r share a SIMD (waves w and w+4): lower-triangle MFMA work is balanced across the SIMDs
  int trow = wv < FT / 2 ? wv : (FT - 1) - (wv - FT / 2);
  if (Tn == FT) {
    // no idle tile row: the wave of row 0 (one tile of update work) also inverts the diagonal tiles, and its SIMD
    // partner takes the next lightest row, so that the inversion chain competes with the fewest MFMAs:
    // SIMD pairs (0, 1), (2, FT-1), (3, FT-2), ...
    trow = wv == 0 ? 0 : wv == FT / 2 ? 1 : wv < FT / 2 ? wv + 1 : FT + FT / 2 - wv;
  }
  const bool live = trow < Tn, ewave = trow == (Tn < FT ? FT - 1 : 0);
  const SweepCtx x{trow, lane, lane & 15, lane >> 4, np, N, live, ewave, bad,
                   (S.prof && blockIdx.x == S.prof_block && lane == 0) ? S.prof + 64 + 5 * wv : nullptr};
  if (!live) {
    if (ewave) sweep_role<-1, true>(S, x, A, N, have_e0, e0);
    else sweep_role<-1, false>(S, x, A, N);
    return;
  }
  switch (trow) {
    case 0:
      if (ewave) sweep_role<0, true>(S, x, A, N);
      else sweep_role<0, false>(S, x, A, N);
      break;
    case 1: sweep_role<1, false>(S, x, A, N); break;
    case 2: sweep_role<2, false>(S, x, A, N); break;
    case 3: sweep_role<3, false>(S, x, A, N); break;
    case 4: sweep_role<4, false>(S, x, A, N); break;
    case 5: sweep_role<5, false>(S, x, A, N); break;
    case 6: sweep_role<6, false>(S, x, A, N); break;
    default: sweep_role<7, false>(S, x, A, N); break;
  }
}
#pragma clang fp contract(off)
}  // namespace kslam
