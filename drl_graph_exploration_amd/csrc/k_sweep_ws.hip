// The sweep of the pose-chain solver's landmark system when it lives in the HBM / L2 workspace (> 63 landmarks): sweep_ws, with
// its scalar-pivot tile inversion (inv16) and tile update (tile_step16).  Included and called by k_slam_arrow.hip only.
#pragma once
#include "k_sweep.hip"
namespace kslam {
#pragma clang fp contract(fast)
// ---- in-wave 16 x 16 symmetric inversion: scalar Gauss-Jordan sweeps in registers ----
// d (accumulator layout: lane (lr, lc), reg r = D[lr + 4 r][lc], full symmetric tile K of the system) <- -D^-1; pivots
// 16 K + k >= np are skipped (identity).  Per pivot k: row k is broadcast to the four 16-lane rows with the gfx950
// permlane swaps, the column entries of a lane's rows and the pivot come from DPP row broadcasts: no LDS, no shuffles
// through memory - this dependent chain (16 reciprocals) is the critical path of the whole factorisation.
//
// One scalar pivot.  (xr, q) = (row k broadcast to every lane's column, 1 / D[k][k]) come from the previous step: the
// register that holds row k + 1 is updated first and the next pivot's broadcast + reciprocal chain is started from it,
// so that the rest of this pivot's update runs in the shadow of that chain.  ~50 VALU instructions per pivot at 4 cycles
// each is the floor of this formulation (wave64 on a 16-lane SIMD).
template <int k>
__device__ __forceinline__ void gj_update_reg(const SweepCtx &x, v4d &d, int r, double t, double q) {
  constexpr int rk = k >> 2, lk = k & 3;
  const bool colk = x.lc == k, rowk = x.lr == lk;
  const double c = row_bcast_lane<k>(d[r]);  // D[lr + 4 r][k]
  double v = fma(-c, t, d[r]);
  v = colk ? c * q : v;
  if (r == rk) v = rowk ? (colk ? -q : t) : v;
  d[r] = v;
}
template <int k>
__device__ __forceinline__ void gj_head(const SweepCtx &x, const v4d &d, double &xr, double &q) {
  constexpr int rk = k >> 2, lk = k & 3;
  xr = rowgroup_bcast<lk>(d[rk]);                    // D[k][lc]
  const double p = readlane_f64(d[rk], 16 * lk + k);  // D[k][k] (uniform; off the broadcast chain)
  q = fast_rcp(p);
  if (x.lane == 0 && !(p > 0)) x.bad[0] = 1;
}
template <int k, bool kChainNext>
__device__ __forceinline__ void gj_pivot(const SweepCtx &x, v4d &d, double &xr, double &q) {
  const double t = xr * q, qk = q;
  constexpr int rn = (k + 1 < 16) ? ((k + 1) >> 2) : 0;
  gj_update_reg<k>(x, d, rn, t, qk);
  if constexpr (kChainNext && k + 1 < 16) gj_head<k + 1>(x, d, xr, q);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r != rn) gj_update_reg<k>(x, d, r, t, qk);
}
template <int k = 0>
__device__ __forceinline__ void inv16_masked(const SweepCtx &x, int K, v4d &d) {
  if constexpr (k < 16) {
    if (16 * K + k < x.np) {
      double xr, q;
      gj_head<k>(x, d, xr, q);
      gj_pivot<k, false>(x, d, xr, q);
      inv16_masked<k + 1>(x, K, d);
    }
  }
}
template <int k = 0>
__device__ __forceinline__ void inv16_full(const SweepCtx &x, v4d &d, double &xr, double &q) {
  if constexpr (k < 16) {
    gj_pivot<k, true>(x, d, xr, q);
    inv16_full<k + 1>(x, d, xr, q);
  }
}
__device__ __forceinline__ void inv16(const SweepCtx &x, int K, v4d &d) {
  // all 16 pivots active (every block but the last): one straight-line block, so that the scheduler can start pivot
  // k + 1's broadcast / reciprocal chain under the tail of pivot k's update
  if (16 * K + 16 <= x.np) {
    double xr, q;
    gj_head<0>(x, d, xr, q);
    inv16_full<0>(x, d, xr, q);
  } else {
    inv16_masked<0>(x, K, d);
  }
}

// ---- one lower tile of a block step from row-major KS panels (ks16: k_sweep.hip) ----
// the part of a block step that overwrites instead of updating: tile column K takes -W, the pivot rows -(W)^T, the pivot
// block E_K (masked rows / columns excepted)
__device__ __forceinline__ void tile_replace16(int I, int J, int K, int np, int lc, int lr, const double *wt, const double *einv,
                                               v4d &acc) {
  const int kb = 16 * K;
  if (I > K && J == K) {  // A_IK <- A_IK D^-1 (masked columns: W = 0)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = -wt[(16 * I + lr + 4 * r) * 16 + ks16(lc)];
  }
  if (I == K) {
    if (J < K) {  // pivot rows: A_KJ <- -(W_J)^T; rows >= np (rhs, pads) keep the regular update
      double tt[4];
      ld4(wt + (16 * J + lc) * 16 + lr * 4, tt);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = (kb + lr + 4 * r < np) ? -tt[r] : acc[r];
    } else {  // pivot block <- E_K; masked rows / columns take -W like any other row
      double ee[4], tt[4];
      ld4(einv + lc * 16 + lr * 4, ee);
      ld4(wt + (16 * K + lc) * 16 + lr * 4, tt);
      const bool colact = kb + lc < np;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool rowact = kb + lr + 4 * r < np;
        const double wv = wt[(16 * K + lr + 4 * r) * 16 + ks16(lc)];
        acc[r] = rowact ? (colact ? ee[r] : -tt[r]) : (colact ? -wv : acc[r]);
      }
    }
  }
}

// One lower tile (I, J) of block step K of the 16-wide symmetric sweep: the update / replacement rules above, from the
// panels PAN (pivot column), WT = PAN E_K and E_K.  acc: accumulator layout (row lr + 4 r, column lc of the tile; diagonal tiles fully symmetric).
__device__ __forceinline__ void tile_step16(int I, int J, int K, int np, int lc, int lr, const double *pan, const double *wt,
                                            const double *einv, v4d &acc) {
  const int kb = 16 * K;
  const bool has_mask = np < kb + 16;
  if ((I != K || has_mask) && (J != K || I == K)) {
    double aW[4], bP[4];
    ld4(wt + (16 * I + lc) * 16 + lr * 4, aW);
    ld4(pan + (16 * J + lc) * 16 + lr * 4, bP);
    acc = mfma4(aW, bP, acc);
  }
  tile_replace16(I, J, K, np, lc, lr, wt, einv, acc);
}

// tile t of the lower triangle, counted row by row -> its tile row / column
__device__ __forceinline__ void tile_of(int t, int &ib, int &jb) {
  ib = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
  while ((ib + 1) * (ib + 2) / 2 <= t) ++ib;
  while (ib * (ib + 1) / 2 > t) --ib;
  jb = t - ib * (ib + 1) / 2;
}

// Symmetric Gauss-Jordan sweep of the square matrix `A` in the workspace (leading dimension N = 16 Tn, lower triangle valid) on
// the pivots [0, np); rows >= np (the rhs row np, pads) are carried along.  Afterwards the lower triangle holds -A_pp^-1 and row
// np the solution.  All kThreads threads call it.  The block steps of k_sweep.hip (P / W / U / look-ahead) with row-major KS
// panels and three barriers per step: seven waves own the lower tiles (tile t: wave t mod 7), the eighth inverts the diagonal
// tiles.  NTW says where a wave's tiles live between the block steps:
//   NTW > 0   in NTW accumulator tiles per wave (<= 7 NTW tiles: <= 127 landmarks at NTW = 20); `pan` / `wt` (16 N doubles
//             each) are LDS, the pivot column panel is published from the registers
//   NTW == 0  in the workspace, like `pan` / `wt`: every lower tile is read, updated and written back once per block step
//             (8 bytes x N^2 / 2 per step - a few hundred MB per update at 500 landmarks; the reference has no landmark cap,
//             SLAM2D.cpp:103-124: this form exists so that such worlds RUN, not to be fast)
// lds_s: 1280 doubles of LDS - the two E tiles, the dump of the next diagonal tile, the look-ahead's layout scratch.
template <int NTW>
__device__ __forceinline__ void sweep_ws(double *A, double *pan, double *wt, double *lds_s, int np, int N, int Tn, int *bad, int tid) {
  constexpr bool kResident = NTW > 0;
  constexpr int NA = kResident ? NTW : 1, TW = kWaves - 1;
  const int ld = N, ntiles = Tn * (Tn + 1) / 2;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lc = lane & 15, lr = lane >> 4;
  const bool ewave = wave == TW;
  double *einv0 = lds_s, *dscr = lds_s + 512, *es = dscr + 256;
  const SweepCtx x{0, lane, lc, lr, np, N, true, ewave, bad, nullptr};
  // element (i, j) of the symmetric matrix from its stored lower triangle
  auto sym = [&](int i, int j) -> double { return A[(size_t)max(i, j) * ld + min(i, j)]; };
  // this lane's part of tile (ib, jb) in accumulator layout (diagonal tiles are kept fully symmetric in registers) and back
  auto ld_tile = [&](int ib, int jb, v4d &acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = sym(16 * ib + lr + 4 * r, 16 * jb + lc);
  };
  auto st_tile = [&](int ib, int jb, const v4d &acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * ib + lr + 4 * r, j = 16 * jb + lc;
      if (j <= i) A[(size_t)i * ld + j] = acc[r];
    }
  };
  v4d acc[NA];  // (kResident) tile wave + TW u
  int tI[NA], tJ[NA];
  bool live[NA];
  if constexpr (kResident) {
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
      const int t = wave + TW * u;
      live[u] = !ewave && t < ntiles;
      tI[u] = tJ[u] = 0;
      acc[u] = v4d{0.0, 0.0, 0.0, 0.0};
      if (live[u]) {
        tile_of(t, tI[u], tJ[u]);
        ld_tile(tI[u], tJ[u], acc[u]);
      }
    }
  }
  // E_0 from the first diagonal tile
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dscr[4 * lane + r] = sym(lr + 4 * r, lc);
  }
  __syncthreads();
  if (ewave) {
    double t4[4];
    ld4(dscr + 4 * lane, t4);
    v4d d = {t4[0], t4[1], t4[2], t4[3]};
    inv16(x, 0, d);
#pragma unroll
    for (int r = 0; r < 4; ++r) einv0[(lr + 4 * r) * 16 + ks16(lc)] = d[r];
  }
  __syncthreads();
  for (int K = 0; 16 * K < np; ++K) {
    const int kb = 16 * K;
    const bool have_next = kb + 16 < np;
    double *einv = einv0 + 256 * (K & 1), *enext = einv0 + 256 * ((K + 1) & 1);
    // P: the pivot column panel PAN[i][.] = A[i][16 K + .] (masked rows / columns as zeros) from the tiles of column K and,
    // transposed, of row K; the current values of the next diagonal tile are dumped for the look-ahead
    if constexpr (kResident) {
#pragma unroll
      for (int u = 0; u < NTW; ++u) {
        if (!live[u]) continue;
        if (tJ[u] == K) {
          const bool colact = kb + lc < np;
#pragma unroll
          for (int r = 0; r < 4; ++r) pan[(16 * tI[u] + lr + 4 * r) * 16 + ks16(lc)] = colact ? acc[u][r] : 0.0;
        } else if (tI[u] == K) {  // tJ < K: PAN[16 J + lc][c = lr + 4 r] = A[kb + lr + 4 r][16 J + lc]
          double *o = pan + (16 * tJ[u] + lc) * 16 + lr * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (kb + lr + 4 * r < np) ? acc[u][r] : 0.0;
        }
        if (have_next && tI[u] == K + 1 && tJ[u] == K + 1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) dscr[4 * lane + r] = acc[u][r];
        }
      }
    } else if (!ewave) {
      for (int I = wave; I < Tn; I += TW) {
        if (I >= K) {
          const bool colact = kb + lc < np;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * I + lr + 4 * r;
            pan[(size_t)i * 16 + ks16(lc)] = colact ? sym(i, kb + lc) : 0.0;
          }
        } else {  // PAN[16 I + lc][c = lr + 4 r] = A[kb + lr + 4 r][16 I + lc]
          double *o = pan + (size_t)(16 * I + lc) * 16 + lr * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (kb + lr + 4 * r < np) ? A[(size_t)(kb + lr + 4 * r) * ld + 16 * I + lc] : 0.0;
        }
      }
    } else if (have_next) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dscr[4 * lane + r] = sym(kb + 16 + lr + 4 * r, kb + 16 + lc);
    }
    __syncthreads();
    v4d dn = {0.0, 0.0, 0.0, 0.0};
    if (!ewave) {
      for (int I = wave; I < Tn; I += TW) {  // W_I = PAN_I E_K
        double aP[4], eB[4];
        ld4(pan + (16 * I + lc) * 16 + lr * 4, aP);
        ld4(einv + lc * 16 + lr * 4, eB);
        v4d w = {0.0, 0.0, 0.0, 0.0};
        w = mfma4(aP, eB, w);
#pragma unroll
        for (int r = 0; r < 4; ++r) wt[(16 * I + lr + 4 * r) * 16 + ks16(lc)] = w[r];
      }
    } else if (have_next) {  // look-ahead: D'_{K+1} (the E-wave forms W_{K+1} itself)
      double aP[4], eB[4], aW[4], t4[4];
      ld4(pan + (16 * (K + 1) + lc) * 16 + lr * 4, aP);  // also the B operand of the update (PAN_{K+1}^T)
      ld4(einv + lc * 16 + lr * 4, eB);
      v4d w1 = {0.0, 0.0, 0.0, 0.0};
      w1 = mfma4(aP, eB, w1);
#pragma unroll
      for (int r = 0; r < 4; ++r) es[(lr + 4 * r) * 16 + ks16(lc)] = w1[r];  // accumulator -> A-operand layout
      wave_lds_sync();
      ld4(es + lc * 16 + lr * 4, aW);
      ld4(dscr + 4 * lane, t4);
      dn = v4d{t4[0], t4[1], t4[2], t4[3]};
      dn = mfma4(aW, aP, dn);
    }
    __syncthreads();
    if (ewave) {
      if (have_next) {
        inv16(x, K + 1, dn);
#pragma unroll
        for (int r = 0; r < 4; ++r) enext[(lr + 4 * r) * 16 + ks16(lc)] = dn[r];
      }
    } else if constexpr (kResident) {
#pragma unroll
      for (int u = 0; u < NTW; ++u)
        if (live[u]) tile_step16(tI[u], tJ[u], K, np, lc, lr, pan, wt, einv, acc[u]);
    } else {
      for (int t = wave; t < ntiles; t += TW) {
        int ib, jb;
        tile_of(t, ib, jb);
        v4d a;
        ld_tile(ib, jb, a);
        tile_step16(ib, jb, K, np, lc, lr, pan, wt, einv, a);
        st_tile(ib, jb, a);
      }
    }
    __syncthreads();
  }
  if constexpr (kResident) {
#pragma unroll
    for (int u = 0; u < NTW; ++u)
      if (live[u]) st_tile(tI[u], tJ[u], acc[u]);
  }
}
#pragma clang fp contract(off)
}  // namespace kslam
