// fp32 GEMM on the gfx950 matrix cores, C[M x N] = op(A) op(B) with a fused epilogue; nothing here knows about the GCN (k_gcn.hip
// is its user, scripts/micro/gemm*_bench.hip include this file alone).  Three kernels: k_gemm_dl (64x64, operand tiles global ->
// LDS directly), k_gemm (register-staged, any alignment; same MFMA order as k_gemm_dl), k_gemm_wide (tall tiles, 4 or 8 waves);
// gemm() picks per launch (wide_pick), gemm_tn_splitk() adds split-K with a deterministic second stage.
// Development switches, read once per process: DRLGX_GEMM_DL=0, DRLGX_GEMM_TILE=1, DRLGX_GEMM_WIDE=0 / 6..10.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "drlgx_dev.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// workgroup id -> (row panel tm, column tile tn) of a launch of tiles_n * roundup8(tiles_m) workgroups (x) per K-slice (z); false: no tile.
// XCD-aware order: consecutive workgroup ids go round-robin over the 8 XCDs; XCD x gets the row panels x, x + 8, ... and walks a
// panel's column tiles on consecutive slots (the panel of A stays in its L2).  With fewer row panels than XCDs - the read-out layer's
// weight gradient, M = out_dim rows: ONE panel - that order would put the whole launch on tiles_m XCDs (32 CUs each: 357 us for a
// 4.4 GFLOP product); such launches take the plain order, consecutive tiles on consecutive XCDs.
__device__ __forceinline__ bool tile_of_block(int tiles_m, int tiles_n, int &tm, int &tn) {
  if (tiles_m < 8) {
    tm = blockIdx.x % tiles_m;
    tn = blockIdx.x / tiles_m;
    return tn < tiles_n;
  }
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  tn = slot % tiles_n;
  tm = (slot / tiles_n) * 8 + xcd;
  return tm < tiles_m;
}

// The fused epilogue of every kernel below, at element `at` = row * ldc + col of the [M x ldc] matrices:
// EPI 0: C = acc (split-K partial when gridDim.z > 1: C += z * M * N)
// EPI 1: C = relu(acc + bias[col]) * (mask ? mask[row][col] : 1)        (forward layer 2)
// EPI 2: C = acc + bias[col]                                            (read-out layer with more than 8 outputs: the critic's 100)
// EPI 3: C = acc * (G[row][col] > 0) * (mask ? mask[row][col] : 1), G = the `bias` argument read as an [M x ldc] matrix
//        (dZ2 of that read-out layer: G = H2, the ReLU gate recovered from it as in k_dz2)
constexpr bool epi_adds_bias(int epi) { return epi == 1 || epi == 2; }  // bj below = bias[col], loaded once per column
constexpr bool epi_reads_mask(int epi) { return epi == 1 || epi == 3; }
template <int EPI>  // on loaded values: b = bias[col] (EPI 1, 2) or G[row][col] (EPI 3); m = mask[row][col] where there is a mask
__device__ __forceinline__ float epilogue(float v, float b, bool masked, float m) {
  if (EPI == 1) {
    v = fmaxf(v + b, 0.f);
    if (masked) v *= m;
  } else if (EPI == 2) {
    v += b;
  } else if (EPI == 3) {
    float g = b > 0.f ? 1.f : 0.f;
    if (masked) g *= m;
    v *= g;
  }
  return v;
}
template <int EPI>  // ... of element `at`
__device__ __forceinline__ float epilogue(float v, float bj, const float *G, const float *mask, size_t at) {
  return epilogue<EPI>(v, EPI == 3 ? G[at] : bj, mask != nullptr, epi_reads_mask(EPI) && mask ? mask[at] : 0.f);
}
template <int EPI>  // ... of four consecutive columns from `at` on: G and the mask by 16-byte loads
__device__ __forceinline__ float4 epilogue(float4 v, float4 bj, const float *G, const float *mask, size_t at) {
  float4 b = bj, m = bj;
  if (EPI == 3) b = *reinterpret_cast<const float4 *>(G + at);
  if (epi_reads_mask(EPI) && mask) m = *reinterpret_cast<const float4 *>(mask + at);
  const bool masked = mask != nullptr;
  return make_float4(epilogue<EPI>(v.x, b.x, masked, m.x), epilogue<EPI>(v.y, b.y, masked, m.y), epilogue<EPI>(v.z, b.z, masked, m.z),
                     epilogue<EPI>(v.w, b.w, masked, m.w));
}

// global -> LDS directly (gfx950): an LDS address as the wave-uniform offset the instruction takes in m0, and one
// global_load_lds_dwordx4 to it - 1 KB per wave.  (Inline assembly: through the builtin the compiler knows that the load writes
// LDS and drains every load in flight - s_waitcnt vmcnt(0) - before the next LDS read, which is exactly the overlap the DMA
// kernels are about; m0 is not otherwise used in them: gfx9 LDS instructions do not read it.)
__device__ __forceinline__ unsigned lds_off(const float *p) {
  return (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(__attribute__((address_space(3))) const void *)p);
}
__device__ __forceinline__ void dma16(const float *g, unsigned lds) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds), "v"(g) : "memory");
}
// k-contiguous operand tile [x][16 k], unpadded, the 16-byte quads of a row XOR-swizzled by (x >> 1) & 3 (conflict-free
// ds_read_b128 over 8 consecutive rows).  Source address of the quad that lands at row x, quad c of the tile (+ k0), and the
// partial last K-tile through registers with zero fill (k >= kend must contribute nothing):
__device__ __forceinline__ const float *kc_src(const float *P, int ld, int x0, int X, int x, int c) {
  return P + (size_t)min(x0 + x, X - 1) * ld + 4 * (c ^ ((x >> 1) & 3));
}
__device__ __forceinline__ void kc_tail(float *T, const float *P, int ld, int x0, int X, int k0, int kend, int x, int c) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k0 + 4 * c < kend) v = *reinterpret_cast<const float4 *>(P + (size_t)min(x0 + x, X - 1) * ld + k0 + 4 * c);
  *reinterpret_cast<float4 *>(T + x * 16 + 4 * (c ^ ((x >> 1) & 3))) = v;
}

// ------------------------------------------------------------------------------------------------
// The same GEMM with the operand tiles loaded global -> LDS directly (global_load_lds_dwordx4, gfx950): no VGPR staging
// and no ds_write instructions, four LDS stages with three tiles in flight.  Bit-identical to k_gemm (same MFMA order);
// 6-10 % faster on the 17 287-row batches, equal on the 4 340-row ones (scripts/micro/gemm_dl_bench.hip).
// ------------------------------------------------------------------------------------------------
constexpr int DL_ST = 4;  // LDS stages: tile t + 3 is in flight while tile t is multiplied

// C[M x N] = op(A) op(B) with the operand tiles loaded global -> LDS directly.  AKC / BKC: the operand's source is
// k-contiguous (A stored [M][K] / B stored [N][K]), else x-contiguous (A stored [K][M] / B stored [K][N]).
//   k-contiguous tile  [64 x][16 k] as kc_src: wave w loads rows 16w .. 16w+15 (lane = 4 row + quad);
//   x-contiguous tile  [16 k][64 x] unpadded: wave w loads k rows 4w .. 4w+3 (lane = 16 k + x quad).
// One global_load_lds_dwordx4 per wave and operand brings 1 KB.  Contract (host): lda, ldb, the contiguous extents and the
// base addresses are multiples of 4 floats; extents >= 4.
template <bool KC>
__device__ __forceinline__ const float *dl_src(const float *P, int ld, int x0, int X, int wave, int lane) {
  if (KC) return kc_src(P, ld, x0, X, 16 * wave + (lane >> 2), lane & 3);  // (+ k0)
  return P + (size_t)(4 * wave + (lane >> 4)) * ld + min(x0 + 4 * (lane & 15), X - 4);  // (+ k0 * ld)
}
template <bool KC>
__device__ __forceinline__ void dl_frag(float (&f)[8], const float *T, int xb, int lane) {
  const int li = lane & 31, h = lane >> 5, x = xb + li;
  if (KC) {
    const int sw = (x >> 1) & 3;
    const float4 u0 = *reinterpret_cast<const float4 *>(T + x * 16 + 4 * ((2 * h) ^ sw));
    const float4 u1 = *reinterpret_cast<const float4 *>(T + x * 16 + 4 * ((2 * h + 1) ^ sw));
    f[0] = u0.x; f[1] = u0.y; f[2] = u0.z; f[3] = u0.w; f[4] = u1.x; f[5] = u1.y; f[6] = u1.z; f[7] = u1.w;
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) f[s] = T[(8 * h + s) * 64 + x];
  }
}
template <bool KC>  // the partial last K-tile
__device__ __forceinline__ void dl_tail(float *T, const float *P, int ld, int x0, int X, int k0, int kend, int tid) {
  if (KC) return kc_tail(T, P, ld, x0, X, k0, kend, tid >> 2, tid & 3);
  const int k = tid >> 4, xq = tid & 15;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k0 + k < kend) v = *reinterpret_cast<const float4 *>(P + (size_t)(k0 + k) * ld + min(x0 + 4 * xq, X - 4));
  *reinterpret_cast<float4 *>(T + k * 64 + 4 * xq) = v;
}

template <bool AKC, bool BKC, int EPI>
__global__ __launch_bounds__(256) void k_gemm_dl(int M, int N, int K, const float *__restrict__ A, int lda, const float *__restrict__ B,
                                                 int ldb, float *__restrict__ C, int ldc, const float *__restrict__ bias,
                                                 const float *__restrict__ mask, int k_per_split, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float As[DL_ST][64 * 16];
  __shared__ __attribute__((aligned(16))) float Bs[DL_ST][16 * 64];
  int tm, tn;
  if (!tile_of_block(tiles_m, tiles_n, tm, tn)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = tm * 64, n0 = tn * 64;
  const int kbeg = blockIdx.z * k_per_split, kend = min(K, kbeg + k_per_split);
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int nfull = (kend - kbeg) / 16, tail = (kend - kbeg) - 16 * nfull;
  const float *ga = dl_src<AKC>(A, lda, m0, M, wave, lane) + (AKC ? (size_t)kbeg : (size_t)kbeg * lda);
  const float *gb = dl_src<BKC>(B, ldb, n0, N, wave, lane) + (BKC ? (size_t)kbeg : (size_t)kbeg * ldb);
  const size_t sa = AKC ? 16 : (size_t)16 * lda, sb = BKC ? 16 : (size_t)16 * ldb;  // source step per K-tile
  auto issue = [&](int t) {
    const int st = t & (DL_ST - 1);
    dma16(ga + sa * t, lds_off(&As[st][wave * 256]));
    dma16(gb + sb * t, lds_off(&Bs[st][wave * 256]));
  };
  auto multiply = [&](int st) {
    float fa[8], fb[8];
    dl_frag<AKC>(fa, As[st], wm * 32, lane);
    dl_frag<BKC>(fb, Bs[st], wn * 32, lane);
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc, 0, 0, 0);
  };
  if (nfull > 0) issue(0);
  if (nfull > 1) issue(1);
  if (nfull > 2) issue(2);
  for (int t = 0; t < nfull; ++t) {
    // tile t has landed when at most the loads of tiles t+1 and t+2 (two instructions each) are still in flight
    if (t + 2 < nfull) __builtin_amdgcn_s_waitcnt(0x0F74);       // vmcnt(4)
    else if (t + 1 < nfull) __builtin_amdgcn_s_waitcnt(0x0F72);  // vmcnt(2)
    else __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0)
    __builtin_amdgcn_s_barrier();  // (no fence: a fence would drain the loads in flight) every wave's part of tile t is in
                                   // LDS; every wave is done with tile t-1, whose buffer is refilled next
    if (t + 3 < nfull) issue(t + 3);
    multiply(t & (DL_ST - 1));
  }
  if (tail > 0) {
    __syncthreads();
    const int st = nfull & (DL_ST - 1), k0 = kbeg + 16 * nfull;
    dl_tail<AKC>(As[st], A, lda, m0, M, k0, kend, tid);
    dl_tail<BKC>(Bs[st], B, ldb, n0, N, k0, kend, tid);
    __syncthreads();
    multiply(st);
  }
  // epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  // (the clamped loads of an edge tile only disturb rows >= M / columns >= N, which are not stored)
  float *Cz = C + (EPI == 0 ? (size_t)blockIdx.z * M * ldc : 0);
  const int col = n0 + wn * 32 + (lane & 31);
  if (col < N) {
    const float bj = epi_adds_bias(EPI) ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
      if (row >= M) continue;
      const size_t at = (size_t)row * ldc + col;
      Cz[at] = epilogue<EPI>(acc[r], bj, bias, mask, at);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// fp32 MFMA GEMM  C[M x N] = op(A) op(B)   (row-major; TA: A is stored [K x M]; TB: B is stored [N x K])
// workgroup tile (64 MI) x (64 NI) x 16, 256 threads = 2x2 waves, each wave MI x NI tiles of v_mfma_f32_32x32x2_f32: the product
// runs MI = NI = 1 (64x64, one tile per wave); DRLGX_GEMM_TILE=1 selects the 64x128 instantiation (NI = 2) for experiments.
//  * global -> registers -> LDS with one 16-byte load/store per quarter tile row (scalar predicated loads only for
//    operands whose contiguous dimension is not a multiple of 4: the [nodes x out_dim] head gradient);
//  * an operand whose source is k-contiguous sits in LDS as [x][k] (stride 20 floats: ds_write_b128 straight from
//    the load, fragment = two conflict-free ds_read_b128); an x-contiguous one as [k][x] (stride 64 XR + 4, ds_read_b32);
//  * MFMA step s of a K-tile multiplies k = s (lanes 0-31) and k = 8 + s (lanes 32-63) - any pairing of the 16 k's is
//    a valid 32x32x2 schedule, and this one makes each lane's 8 fragment values contiguous in the [x][k] layout;
//  * the fragments of a K-tile are read during the MFMAs of the one before it, so that its 8 MI NI MFMAs issue back to back
//    while the next tiles' global loads are in flight; one barrier per K-tile (three LDS buffers);
//  * workgroup id -> tile: tile_of_block; epilogue: EPI as at epilogue().
// ------------------------------------------------------------------------------------------------
constexpr int BK = 16;
constexpr int LDK = BK + 4;  // [x][k] tile stride (floats)

// LDS footprint of one operand tile of XR * 64 rows/cols (either layout)
template <int XR>
struct TileF {
  static constexpr int ldx = XR * 64 + 4;  // [k][x] tile stride
  static constexpr int value = (XR * 64 * LDK > BK * ldx) ? XR * 64 * LDK : BK * ldx;
};

// quarter-tile loads of one operand tile (XR * 64 x 16): KC = source is k-contiguous (src[x * ld + k]), else
// src[k * ld + x]; 256 threads move XR float4 each
template <bool KC, bool VEC, int XR>
__device__ __forceinline__ void g_load(float4 (&reg)[XR], bool (&okr)[XR], const float *__restrict__ src, int ld, int x0, int X,
                                       int k0, int kend, int tid) {
#pragma unroll
  for (int r = 0; r < XR; ++r) {
    const int x = KC ? x0 + (tid >> 2) + 64 * r : (XR == 2 ? x0 + (tid & 31) * 4 : x0 + (tid & 15) * 4);
    const int k = KC ? k0 + (tid & 3) * 4 : (XR == 2 ? k0 + (tid >> 5) + 8 * r : k0 + (tid >> 4));
    if (VEC) {
      // contract (host): the contiguous dimension, ld and the base address are multiples of 4 floats, so a float4
      // is all inside or all outside; outside ones load a clamped (valid) address unconditionally and are zeroed
      // when they are stored to LDS (so that nothing waits on the load before the MFMAs of the current tile)
      okr[r] = x < X && k < kend;
      const int xc = min(x, X - (KC ? 1 : 4)), kc = min(k, kend - (KC ? 4 : 1));
      const size_t at = KC ? (size_t)xc * ld + kc : (size_t)kc * ld + xc;
      reg[r] = *reinterpret_cast<const float4 *>(src + at);
    } else {
      okr[r] = true;
      const size_t at = KC ? (size_t)x * ld + k : (size_t)k * ld + x;
      float e[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool ok = KC ? (x < X && k + c < kend) : (k < kend && x + c < X);
        e[c] = ok ? src[at + c] : 0.f;
      }
      reg[r] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
}

template <bool KC, int XR>
__device__ __forceinline__ void s_store(float *T, const float4 (&reg)[XR], const bool (&okr)[XR], int tid) {
  constexpr int ldx = TileF<XR>::ldx;
#pragma unroll
  for (int r = 0; r < XR; ++r) {
    float *p = KC ? T + ((tid >> 2) + 64 * r) * LDK + (tid & 3) * 4
                  : (XR == 2 ? T + ((tid >> 5) + 8 * r) * ldx + (tid & 31) * 4 : T + (tid >> 4) * ldx + (tid & 15) * 4);
    const float4 v = reg[r];
    const bool ok = okr[r];
    *reinterpret_cast<float4 *>(p) = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
  }
}

// the 8 values lane (li, h) feeds to MFMA steps 0..7 for tile rows/cols xb + li: k = 8 h + s
template <bool KC, int XR>
__device__ __forceinline__ void s_frag(float (&f)[8], const float *T, int xb, int lane) {
  constexpr int ldx = TileF<XR>::ldx;
  const int li = lane & 31, h = lane >> 5;
  if (KC) {
    const float4 u0 = *reinterpret_cast<const float4 *>(T + (xb + li) * LDK + 8 * h);
    const float4 u1 = *reinterpret_cast<const float4 *>(T + (xb + li) * LDK + 8 * h + 4);
    f[0] = u0.x; f[1] = u0.y; f[2] = u0.z; f[3] = u0.w;
    f[4] = u1.x; f[5] = u1.y; f[6] = u1.z; f[7] = u1.w;
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) f[s] = T[(8 * h + s) * ldx + xb + li];
  }
}

// MI x NI = 32x32 sub-tiles per wave; the workgroup tile is (64 MI) x (64 NI)
template <bool TA, bool TB, int EPI, bool AV, bool BV, int MI, int NI>
__global__ __launch_bounds__(256) void k_gemm(
    int M, int N, int K, const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb, float *__restrict__ C, int ldc,
    const float *__restrict__ bias, const float *__restrict__ mask, int k_per_split, int tiles_m, int tiles_n) {
  constexpr int BM = 64 * MI, BN = 64 * NI;
  __shared__ __attribute__((aligned(16))) float As[3][TileF<MI>::value];
  __shared__ __attribute__((aligned(16))) float Bs[3][TileF<NI>::value];
  int tm, tn;
  if (!tile_of_block(tiles_m, tiles_n, tm, tn)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = blockIdx.z * k_per_split, kend = min(K, kbeg + k_per_split);
  floatx16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // software pipeline, per K-tile t (one barrier each):
  //   MFMAs of tile t from fragment registers F[t & 1], and between them
  //     ds_write  staging registers (tile t+2, loaded during t-1)  -> LDS buffer (t+2) % 3
  //     global    loads of tile t+3                                -> staging registers
  //     ds_read   fragments of tile t+1 from LDS buffer (t+1) % 3  -> F[(t+1) & 1]
  // so a wave's LDS and global traffic issues under its own MFMAs (a lone workgroup on a CU - small problems, the
  // tail of large ones - has no co-resident waves to hide it), and the barrier only orders tile t+2's stores
  // before the next step's fragment reads (and this step's reads of buffer (t+1) % 3 before its reuse at t+2).
  float4 ra[MI], rb[NI];
  bool oka[MI], okb[NI];
  float fa[2][MI][8], fb[2][NI][8];
  const int ntile = (kend - kbeg + BK - 1) / BK;
  auto load = [&](int t) {
    g_load<!TA, AV, MI>(ra, oka, A, lda, m0, M, kbeg + t * BK, kend, tid);
    g_load<TB, BV, NI>(rb, okb, B, ldb, n0, N, kbeg + t * BK, kend, tid);
  };
  auto store = [&](int buf) {
    s_store<!TA, MI>(As[buf], ra, oka, tid);
    s_store<TB, NI>(Bs[buf], rb, okb, tid);
  };
  auto frags = [&](int set, int buf) {
#pragma unroll
    for (int i = 0; i < MI; ++i) s_frag<!TA, MI>(fa[set][i], As[buf], wm * 32 * MI + 32 * i, lane);
#pragma unroll
    for (int j = 0; j < NI; ++j) s_frag<TB, NI>(fb[set][j], Bs[buf], wn * 32 * NI + 32 * j, lane);
  };
  auto mfma_steps = [&](int set, int s0, int s1) {
#pragma unroll
    for (int s = s0; s < s1; ++s)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][s], fb[set][j][s], acc[i][j], 0, 0, 0);
  };
  // one pipeline step; `set` is a compile-time constant at both call sites (loop unrolled by two)
  auto step = [&](int set, int t, int b0) {  // b0 = t % 3
    const int b1 = b0 == 2 ? 0 : b0 + 1, b2 = b1 == 2 ? 0 : b1 + 1;
    mfma_steps(set, 0, 2);
    if (t + 2 < ntile) store(b2);
    mfma_steps(set, 2, 4);
    if (t + 3 < ntile) load(t + 3);
    mfma_steps(set, 4, 6);
    if (t + 1 < ntile) frags(set ^ 1, b1);
    mfma_steps(set, 6, 8);
    __syncthreads();
  };
  if (ntile > 0) {
    load(0);
    store(0);
  }
  if (ntile > 1) {
    load(1);
    store(1);
  }
  if (ntile > 2) load(2);
  __syncthreads();
  if (ntile > 0) frags(0, 0);
  int b = 0;
  for (int t = 0; t < ntile; t += 2) {
    step(0, t, b);
    b = b == 2 ? 0 : b + 1;
    if (t + 1 >= ntile) break;
    step(1, t + 1, b);
    b = b == 2 ? 0 : b + 1;
  }
  // epilogue: C/D layout of 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float *Cz = C + (EPI == 0 ? (size_t)blockIdx.z * M * ldc : 0);
  if (m0 + BM <= M && n0 + BN <= N) {  // interior tile: straight-line loads and stores
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = n0 + wn * 32 * NI + j * 32 + (lane & 31);
      const float bj = epi_adds_bias(EPI) ? bias[col] : 0.f;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const size_t at = (size_t)(m0 + wm * 32 * MI + i * 32 + 4 * (lane >> 5)) * ldc + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // rows 8 q + {0, 1, 2, 3} (+ 4 for the upper half wave), their mask rows loaded ahead
          float mk[4];
          if (epi_reads_mask(EPI) && mask) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mk[r] = mask[at + (size_t)(r + 8 * q) * ldc];
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const size_t ar = at + (size_t)(r + 8 * q) * ldc;
            Cz[ar] = epilogue<EPI>(acc[i][j][4 * q + r], EPI == 3 ? bias[ar] : bj, mask != nullptr, mk[r]);
          }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = n0 + wn * 32 * NI + j * 32 + (lane & 31);
    if (col >= N) continue;
    const float bj = epi_adds_bias(EPI) ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 * MI + i * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
        if (row >= M) continue;
        const size_t at = (size_t)row * ldc + col;
        Cz[at] = epilogue<EPI>(acc[i][j][r], bj, bias, mask, at);
      }
  }
}

// ------------------------------------------------------------------------------------------------
// Tall-tile GEMM for the hidden x hidden products of a batch (M or K = the batch's node count).  The 64x64 kernels above
// ask the CU's vector L1 for 16 B per clock and workgroup - 68-80 B/clk at the 4-5 workgroups a CU holds, against the
// 64 B/clk it delivers: 64-75 % of the fp32 MFMA rate is their ceiling.  Here a workgroup of 8 waves owns (16 RT) x 128
// of C (RT = 6 .. 10 row sub-tiles, picked per launch so that the tile count fills whole rounds of 256 CUs):
//  * wave w owns the 16 columns 16 w .. 16 w + 15 of the tile and all its rows: RT accumulators of v_mfma_f32_16x16x4_f32,
//    issued with the operands swapped (D = B^T A^T) so that a lane holds four consecutive columns of one row of C and the
//    epilogue is one 16-byte store (bias / mask one 16-byte load) per sub-tile;
//  * operand tiles global -> LDS directly as in k_gemm_dl (four stages, 16 k per stage), (16 RT + 128) * 64 B per stage:
//    7-8 B per clock and workgroup from the L1;
//  * MFMA step s multiplies k = 4 q + s in lane group q = lane >> 4, so that a k-contiguous operand's fragment is one
//    ds_read_b128 ([x][16 k] rows, quads XOR-swizzled by (x >> 1) & 3: the four 16-lane groups of the read are
//    conflict-free) and an x-contiguous one's four ds_read_b32 ([16 k][W x], 16-float groups of row k XOR-swizzled by
//    (k >> 2) & 1: lane groups q and q + 1 read different bank halves);
//  * a DMA instruction brings 1 KB = 16 rows of a k-contiguous tile (or 256 / W rows of an x-contiguous one); the RT + 8
//    instructions of a stage are dealt round-robin to the 8 waves, and a wave without a real one in a round issues it
//    into a scratch KB (every wave's vmcnt then counts the same number per stage).
// Contract (host): vec_ok() operands and C, x-contiguous A only with 16 RT % 32 == 0.
// ------------------------------------------------------------------------------------------------
constexpr int WD_ST = 4;
template <int RT, int NW>  // RT 16-row sub-tiles x NW waves of 16 columns each
struct WideTile {
  static constexpr int AI = (RT + NW - 1) / NW;                  // A instructions per wave and stage
  static constexpr int stage_floats = (RT + NW) * 256;           // A tile, then B tile
  static constexpr int lds_floats = WD_ST * stage_floats + 256;  // + the scratch KB
};

// source address of DMA instruction j (1 KB = quads 64 j .. 64 j + 63 of the tile) for this lane
template <bool KC>
__device__ __forceinline__ const float *wd_src(const float *P, int ld, int x0, int X, int W, int j, int lane) {
  const int q = 64 * j + lane;
  if (KC) return kc_src(P, ld, x0, X, q >> 2, q & 3);  // (+ k0)
  const int wq = W >> 2, k = q / wq, xq = (q - k * wq) ^ (4 * ((k >> 2) & 1));
  return P + (size_t)k * ld + min(x0 + 4 * xq, X - 4);  // (+ k0 * ld)
}
// the four values lane (i = lane & 15, q = lane >> 4) feeds to MFMA steps 0..3 for tile row / column xb + i: k = 4 q + s
template <bool KC>
__device__ __forceinline__ float4 wd_frag(const float *T, int W, int xb, int lane) {
  const int x = xb + (lane & 15), q = lane >> 4;
  if (KC) return *reinterpret_cast<const float4 *>(T + x * 16 + 4 * (q ^ ((x >> 1) & 3)));
  const float *p = T + (4 * q) * W + (x ^ (16 * (q & 1)));
  return make_float4(p[0], p[W], p[2 * W], p[3 * W]);
}
template <bool KC, int NT>  // the partial last K-tile
__device__ __forceinline__ void wd_tail(float *T, const float *P, int ld, int x0, int X, int W, int k0, int kend, int tid) {
  for (int q = tid; q < 4 * W; q += NT) {
    if (KC) { kc_tail(T, P, ld, x0, X, k0, kend, q >> 2, q & 3); continue; }
    const int wq = W >> 2, k = q / wq, xq = q - k * wq;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k0 + k < kend) v = *reinterpret_cast<const float4 *>(P + (size_t)(k0 + k) * ld + min(x0 + 4 * xq, X - 4));
    *reinterpret_cast<float4 *>(T + k * W + 4 * (xq ^ (4 * ((k >> 2) & 1)))) = v;
  }
}

template <bool AKC, bool BKC, int EPI, int RT, int NW>
__global__ __launch_bounds__(64 * NW) void k_gemm_wide(int M, int N, int K, const float *__restrict__ A, int lda, const float *__restrict__ B,
                                                   int ldb, float *__restrict__ C, int ldc, const float *__restrict__ bias,
                                                   const float *__restrict__ mask, int k_per_split, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) float wd_smem[];
  using WT = WideTile<RT, NW>;
  constexpr int TM = 16 * RT, WD_N = 16 * NW;
  int tm, tn;
  if (!tile_of_block(tiles_m, tiles_n, tm, tn)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = tm * TM, n0 = tn * WD_N;
  const int kbeg = blockIdx.z * k_per_split, kend = min(K, kbeg + k_per_split);
  floatx4 acc[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int nfull = (kend - kbeg) / 16, tail = (kend - kbeg) - 16 * nfull;
  const unsigned lds0 = lds_off(wd_smem);
  constexpr unsigned stage_bytes = WT::stage_floats * sizeof(float);
  // this wave's instructions of a stage: A instruction j = wave + NW i (the scratch KB when j >= RT), B instruction j = wave
  const float *ga[WT::AI];
  unsigned la[WT::AI], la_step[WT::AI];
#pragma unroll
  for (int i = 0; i < WT::AI; ++i) {
    const int j = wave + NW * i;
    const bool real = j < RT;
    ga[i] = wd_src<AKC>(A, lda, m0, M, TM, real ? j : 0, lane) + (AKC ? (size_t)kbeg : (size_t)kbeg * lda);
    la[i] = real ? lds0 + j * 1024u : lds0 + WD_ST * stage_bytes;
    la_step[i] = real ? stage_bytes : 0u;
  }
  const float *gb = wd_src<BKC>(B, ldb, n0, N, WD_N, wave, lane) + (BKC ? (size_t)kbeg : (size_t)kbeg * ldb);
  const unsigned lb = lds0 + (RT + wave) * 1024u;
  const size_t sa = AKC ? 16 : (size_t)16 * lda, sb = BKC ? 16 : (size_t)16 * ldb;  // source step per K-tile
  constexpr int PER = WT::AI + 1;  // DMA instructions of this wave per stage
  const unsigned scratch = lds0 + WD_ST * stage_bytes;
  // DMA instruction n (0 .. PER - 1) of K-tile t; past the last full tile it re-reads that tile into the scratch KB, so that
  // every step issues PER instructions and one vmcnt value is right throughout
  auto dma = [&](int n, int t) {
    const bool live = t < nfull;
    const int ts = live ? t : nfull - 1;
    const unsigned st = (unsigned)(t & (WD_ST - 1));
    if (n < WT::AI) dma16(ga[n] + sa * ts, live ? la[n] + st * la_step[n] : scratch);
    else dma16(gb + sb * ts, live ? lb + st * stage_bytes : scratch);
  };
  // K-tile t is multiplied from registers; between its MFMAs (one filler behind each of the first few, in the shadow of the
  // MFMA pipe) the wave issues its DMA instructions of tile t + 4 into the stage tile t just left and reads the fragments
  // of tile t + 1.  The barrier at the top (tile t + 1 complete in LDS, every wave has tile t in registers) is followed by
  // MFMAs that wait for nothing.
  float4 fa0[RT], fa1[RT], fb0, fb1;
  auto step = [&](int t, const float4 (&fa)[RT], const float4 &fb, float4 (&na)[RT], float4 &nb) {
    __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * PER));  // tiles t + 2 and t + 3 may still be in flight
    __builtin_amdgcn_s_barrier();
    const float *As = wd_smem + ((t + 1) & (WD_ST - 1)) * WT::stage_floats, *Bs = As + RT * 256;
    const float bs[4] = {fb.x, fb.y, fb.z, fb.w};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float as[4] = {fa[i].x, fa[i].y, fa[i].z, fa[i].w};
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(bs[s], as[s], acc[i], 0, 0, 0);
        const int n = s * RT + i;
        __builtin_amdgcn_sched_barrier(0);
        if (n < PER) dma(n, t + 4);
        else if (n == PER) nb = wd_frag<BKC>(Bs, WD_N, 16 * wave, lane);
        else if (n <= PER + RT) na[n - PER - 1] = wd_frag<AKC>(As, TM, 16 * (n - PER - 1), lane);
        if (n <= PER + RT) __builtin_amdgcn_sched_barrier(0);
      }
  };
  if (nfull > 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int n = 0; n < PER; ++n) dma(n, t);
    __builtin_amdgcn_s_waitcnt(0x0F70 | (3 * PER));
    __builtin_amdgcn_s_barrier();
    fb0 = wd_frag<BKC>(wd_smem + RT * 256, WD_N, 16 * wave, lane);
#pragma unroll
    for (int i = 0; i < RT; ++i) fa0[i] = wd_frag<AKC>(wd_smem, TM, 16 * i, lane);
  }
  for (int t = 0; t < nfull; t += 2) {
    step(t, fa0, fb0, fa1, fb1);
    if (t + 1 >= nfull) break;
    step(t + 1, fa1, fb1, fa0, fb0);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // the scratch re-reads of the last steps (LDS must not be written after the workgroup ends)
  auto read = [&](float4 (&fa)[RT], float4 &fb, int st) {
    const float *As = wd_smem + st * WT::stage_floats, *Bs = As + RT * 256;
    fb = wd_frag<BKC>(Bs, WD_N, 16 * wave, lane);
#pragma unroll
    for (int i = 0; i < RT; ++i) fa[i] = wd_frag<AKC>(As, TM, 16 * i, lane);
  };
  auto multiply = [&](const float4 (&fa)[RT], const float4 &fb) {
    const float bs[4] = {fb.x, fb.y, fb.z, fb.w};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float as[4] = {fa[i].x, fa[i].y, fa[i].z, fa[i].w};
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(bs[s], as[s], acc[i], 0, 0, 0);
      }
  };
  if (tail > 0) {
    __syncthreads();
    const int st = nfull & (WD_ST - 1), k0 = kbeg + 16 * nfull;
    float *As = wd_smem + st * WT::stage_floats;
    wd_tail<AKC, 64 * NW>(As, A, lda, m0, M, TM, k0, kend, tid);
    wd_tail<BKC, 64 * NW>(As + RT * 256, B, ldb, n0, N, WD_N, k0, kend, tid);
    __syncthreads();
    read(fa0, fb0, st);
    multiply(fa0, fb0);
  }
  // D = (B^T A^T) sub-tile: lane holds C[m0 + 16 i + (lane & 15)][n .. n + 3], n = n0 + 16 wave + 4 (lane >> 4)
  float *Cz = C + (EPI == 0 ? (size_t)blockIdx.z * M * ldc : 0);
  const int n = n0 + 16 * wave + 4 * (lane >> 4);
  if (n < N) {
    float4 bj = make_float4(0.f, 0.f, 0.f, 0.f);
    if (epi_adds_bias(EPI)) bj = *reinterpret_cast<const float4 *>(bias + n);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int m = m0 + 16 * i + (lane & 15);
      if (m >= M) continue;
      const size_t at = (size_t)m * ldc + n;
      *reinterpret_cast<float4 *>(Cz + at) = epilogue<EPI>(make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]), bj, bias, mask, at);
    }
  }
}

// deterministic second stage of split-K: out = sum_z part[z]
__global__ void k_splitk_reduce(int n, int S, const float *part, float *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int z = 0; z < S; ++z) s += part[(size_t)z * n + i];
  out[i] = s;
}

bool vec_ok(const float *p, int ld, int contiguous_dim) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0 && (contiguous_dim & 3) == 0;
}

// workgroup tile of the small-product kernels: 64x64 (four waves of 32x32), best or equal among the register-staged tilings
// on every GCN shape; DRLGX_GEMM_TILE=1 selects the 64x128 variant for experiments.  (Large products: gemm_wide below.)
int pick_tile() {
  static const int v = [] {
    const char *e = getenv("DRLGX_GEMM_TILE");
    return e ? atoi(e) : 2;
  }();
  return v;
}

// DRLGX_GEMM_DL=0 keeps the register-staged kernel (A/B runs)
bool gemm_direct_to_lds() {
  static const bool v = [] {
    const char *e = std::getenv("DRLGX_GEMM_DL");
    return !(e && e[0] == '0');
  }();
  return v;
}

// grid of an M x N product in K-slices of kps on (rows x cols) tiles: tile_of_block's tiles_n * roundup8(tiles_m) workgroups per slice
struct GemmGrid {
  int tiles_m, tiles_n; dim3 grid;
};
GemmGrid gemm_grid(int M, int N, int K, int kps, int rows, int cols) {
  const int tiles_m = (M + rows - 1) / rows, tiles_n = (N + cols - 1) / cols;
  return {tiles_m, tiles_n, dim3(tiles_n * ((tiles_m + 7) / 8) * 8, 1, (K + kps - 1) / kps)};
}

template <bool TA, bool TB, int EPI, int MI, int NI>
void gemm_tile(hipStream_t st, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
               const float *bias, const float *mask, int kps) {
  const GemmGrid g = gemm_grid(M, N, K, kps, 64 * MI, 64 * NI);
  const bool avec = vec_ok(A, lda, TA ? M : K), bvec = vec_ok(B, ldb, TB ? K : N);
  if (MI == 1 && NI == 1 && avec && bvec && (TA ? M : K) >= 4 && (TB ? K : N) >= 4 && M >= 1 && N >= 4 && gemm_direct_to_lds()) {
    hipLaunchKernelGGL((k_gemm_dl<!TA, TB, EPI>), g.grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, bias, mask, kps, g.tiles_m, g.tiles_n);
    return;
  }
#define DRLGX_GEMM(AV, BV)                                                                                                     \
  hipLaunchKernelGGL((k_gemm<TA, TB, EPI, AV, BV, MI, NI>), g.grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, bias, mask, \
                     kps, g.tiles_m, g.tiles_n)
  if (avec && bvec) DRLGX_GEMM(true, true);
  else DRLGX_GEMM(false, false);
#undef DRLGX_GEMM
}

// DRLGX_GEMM_WIDE=0 keeps the 64x64 kernels everywhere (A/B runs); DRLGX_GEMM_WIDE=6..10 pins the tile height
int gemm_wide_mode() {
  static const int v = [] {
    const char *e = std::getenv("DRLGX_GEMM_WIDE");
    return e ? atoi(e) : -1;
  }();
  return v;
}

template <bool TA, bool TB, int EPI, int RT, int NW = 8>
void gemm_wide_launch(hipStream_t st, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
                      const float *bias, const float *mask, int kps) {
  const GemmGrid g = gemm_grid(M, N, K, kps, 16 * RT, 16 * NW);
  constexpr int lds = WideTile<RT, NW>::lds_floats * (int)sizeof(float);
  static bool attr_set[32] = {false};
  const void *fns[] = {reinterpret_cast<const void *>(&k_gemm_wide<!TA, TB, EPI, RT, NW>)};
  drlgx_ensure_lds_attr(attr_set, fns, 1, lds);
  hipLaunchKernelGGL((k_gemm_wide<!TA, TB, EPI, RT, NW>), g.grid, dim3(64 * NW), lds, st, M, N, K, A, lda, B, ldb, C, ldc, bias, mask, kps,
                     g.tiles_m, g.tiles_n);
}

// Tile of an M x N product in S K-slices: rt 16-row sub-tiles x nw waves of 16 columns, or rt = 0 for the 64x64 kernels.
//  * enough 128-row x 128-column tiles to occupy half the chip: 8 waves, the height whose tile count wastes least of the last
//    round of 256 CUs (measured order at 4 340 and 17 288 rows: profiles/r04_ab_gemm_tall_tiles.txt);
//  * else, if the 64x64 tiles would not fit one round of 256 CUs: 4 waves x 64 columns, same rule (the 1 000 - 2 000-node
//    mini-batches of the DQN loop: 96 x 64 tiles fill the chip once where 64 x 64 ones need a second, thin round);
//  * else the 64x64 kernels.
struct WidePick {
  int rt, nw;
};
WidePick wide_pick(int M, int N, int S, bool ta) {
  const int mode = gemm_wide_mode();
  if (mode == 0) return {0, 0};
  auto best_rt = [&](int nw) {
    int best = 0;
    long best_cost = 0;
    for (int rt = 6; rt <= (nw == 8 ? 10 : 8); ++rt) {  // (4 waves: one round of 96 / 112 / 128-row tiles covers every size that gets here)
      if (ta && (rt & 1)) continue;  // x-contiguous A: whole 32-float swizzle blocks
      if (mode >= 6 && mode <= 10 && !(ta && (mode & 1)) && rt != mode) continue;
      const long tiles = (long)((M + 16 * rt - 1) / (16 * rt)) * ((N + 16 * nw - 1) / (16 * nw)) * S;
      const long cost = ((tiles + 255) / 256) * rt;
      if (!best || cost <= best_cost) best = rt, best_cost = cost;
    }
    return best;
  };
  if ((long)((M + 127) / 128) * ((N + 127) / 128) * S >= 128) return {best_rt(8), 8};
  if (!ta && (long)((M + 63) / 64) * ((N + 63) / 64) * S > 256 && (long)((M + 95) / 96) * ((N + 63) / 64) * S >= 128) return {best_rt(4), 4};
  return {0, 0};
}

template <bool TA, bool TB, int EPI>
bool gemm_wide(hipStream_t st, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, const float *bias,
               const float *mask, int kps) {
  if (!vec_ok(A, lda, TA ? M : K) || !vec_ok(B, ldb, TB ? K : N) || !vec_ok(C, ldc, N)) return false;
  if ((epi_adds_bias(EPI) && !vec_ok(bias, 4, 4)) || (EPI == 3 && !vec_ok(bias, ldc, N)) ||
      (epi_reads_mask(EPI) && mask && !vec_ok(mask, ldc, N)) || (TA ? M : K) < 4 || (TB ? K : N) < 4 || kps < 16) return false;
  const WidePick pick = wide_pick(M, N, (K + kps - 1) / kps, TA);
#define DRLGX_WIDE(RT, NW)                                                                          \
  case RT:                                                                                          \
    gemm_wide_launch<TA, TB, EPI, RT, NW>(st, M, N, K, A, lda, B, ldb, C, ldc, bias, mask, kps); \
    return true
  if (pick.nw == 8) {
    switch (pick.rt) {
      DRLGX_WIDE(6, 8);
      DRLGX_WIDE(8, 8);
      DRLGX_WIDE(10, 8);
      default: break;
    }
    if constexpr (!TA) {
      switch (pick.rt) {
        DRLGX_WIDE(7, 8);
        DRLGX_WIDE(9, 8);
        default: break;
      }
    }
  }
  if constexpr (!TA) {
    if (pick.nw == 4) {
      switch (pick.rt) {
        DRLGX_WIDE(6, 4);
        DRLGX_WIDE(7, 4);
        DRLGX_WIDE(8, 4);
        default: break;
      }
    }
  }
#undef DRLGX_WIDE
  return false;
}

template <bool TA, bool TB, int EPI>
void gemm(hipStream_t st, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, const float *bias,
          const float *mask, int splits) {
  const int kps = ((K + splits - 1) / splits + BK - 1) / BK * BK;
  if (gemm_wide<TA, TB, EPI>(st, M, N, K, A, lda, B, ldb, C, ldc, bias, mask, kps)) return;
  if (pick_tile() == 1) gemm_tile<TA, TB, EPI, 1, 2>(st, M, N, K, A, lda, B, ldb, C, ldc, bias, mask, kps);
  else gemm_tile<TA, TB, EPI, 1, 1>(st, M, N, K, A, lda, B, ldb, C, ldc, bias, mask, kps);
}

// weight-gradient GEMM  C[M x N] = A^T B with K = #nodes: split-K (enough splits to fill the chip) + deterministic reduce
// max_splits: 8 for the hidden x hidden gradients (the partials' workspace holds eight of them); the thin read-out gradient
// (M = out_dim rows: 32 tiles) takes more slices to reach every CU
void gemm_tn_splitk(hipStream_t st, float *part, size_t part_floats, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                    float *C, int max_splits = 8) {
  const long tiles = (long)((M + 63) / 64) * ((N + 63) / 64);
  int splits = (int)std::min<size_t>(max_splits, part_floats / ((size_t)M * N));
  splits = std::max(1, std::min({splits, (int)((1024 + tiles - 1) / tiles), (K + 255) / 256}));
  const int kps = ((K + splits - 1) / splits + BK - 1) / BK * BK;
  const int S = (K + kps - 1) / kps;
  if (S == 1) {
    gemm<true, false, 0>(st, M, N, K, A, lda, B, ldb, C, N, nullptr, nullptr, 1);
    return;
  }
  if (max_splits > 8)  // thin M: 64 x 64 tiles (the tall tile is slower here: profiles/r04_ab_gemm_tall_tiles.txt)
    gemm_tile<true, false, 0, 1, 1>(st, M, N, K, A, lda, B, ldb, part, N, nullptr, nullptr, kps);
  else
    gemm<true, false, 0>(st, M, N, K, A, lda, B, ldb, part, N, nullptr, nullptr, S);
  hipLaunchKernelGGL(k_splitk_reduce, dim3((M * N + 255) / 256), dim3(256), 0, st, M * N, S, part, C);
}

}  // namespace
