// One-pass (HBM-bound) kernels of the GCN for products with at most 8 rows or columns, where a matrix-core tile would be empty:
// the thin weight gradients with the bias gradients as an extra row, and the read-out layer of up to kThinOut outputs.
#pragma once
#include <algorithm>

#include "k_gemm.hip"  // k_splitk_reduce

namespace {

// tail of k_thin_tn_part / k_dz2_sums: the four waves' sums (rows m < M, and the column-sum row 8) added in a fixed order through
// LDS by wave 0, which writes them to part[blockIdx.y][M + 1][N] at columns n .. n + 3
__device__ __forceinline__ void thin_part_finish(float4 (&acc)[9], float4 (&red)[3][9][64], int M, int N, int n, bool col_ok, float *part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave > 0) {
#pragma unroll
    for (int m = 0; m < 9; ++m)
      if (m < M || m == 8) red[wave - 1][m][lane] = acc[m];
  }
  __syncthreads();
  if (wave > 0 || !col_ok) return;
#pragma unroll
  for (int m = 0; m < 9; ++m)
    if (m < M || m == 8) {
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        const float4 o = red[w][m][lane];
        acc[m].x += o.x; acc[m].y += o.y; acc[m].z += o.z; acc[m].w += o.w;
      }
    }
  float *o = part + (size_t)blockIdx.y * (M + 1) * N + n;
#pragma unroll
  for (int m = 0; m < 8; ++m)
    if (m < M) *reinterpret_cast<float4 *>(o + (size_t)m * N) = acc[m];
  *reinterpret_cast<float4 *>(o + (size_t)M * N) = acc[8];
}

// thin-M products  out[m][n] = sum_k A[k][m] B[k][n]  (m < M <= 8; A stored [K x lda]) plus, as row M, the column sums
// of B: one pass over B (HBM-bound).  A workgroup owns 256 adjacent columns (a lane 4 of them; N % 4 == 0) of the K-slice
// blockIdx.y; its four waves take every fourth row of the slice and are summed in a fixed order through LDS (one wave per
// slice walked 34 rows at 4 340 nodes with half the chip idle: 14.5 us per call, three calls per train step);
// partials -> part[y][M + 1][N]
__global__ __launch_bounds__(256) void k_thin_tn_part(int K, int N, int M, const float *__restrict__ A, int lda,
                                                      const float *__restrict__ B, int ldb, float *__restrict__ part,
                                                      int rows_per_block) {
  __shared__ float4 red[3][9][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = (blockIdx.x * 64 + lane) * 4;
  const bool col_ok = n < N;
  const int k0 = blockIdx.y * rows_per_block, k1 = min(K, k0 + rows_per_block);
  float4 acc[9];
#pragma unroll
  for (int m = 0; m < 9; ++m) acc[m] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col_ok)
    for (int k = k0 + wave; k < k1; k += 4) {
      const float4 b = *reinterpret_cast<const float4 *>(B + (size_t)k * ldb + n);
      const float *a = A + (size_t)k * lda;  // wave-uniform: scalar loads
#pragma unroll
      for (int m = 0; m < 8; ++m)
        if (m < M) {
          const float am = a[m];
          acc[m].x += am * b.x; acc[m].y += am * b.y; acc[m].z += am * b.z; acc[m].w += am * b.w;
        }
      acc[8].x += b.x; acc[8].y += b.y; acc[8].z += b.z; acc[8].w += b.w;
    }
  thin_part_finish(acc, red, M, N, n, col_ok, part);
}

// second stage (deterministic): rows < rows_w of the [M x N] product -> outW, the column-sum row -> outB (either may
// be null). 64 outputs per workgroup, the S partials of each summed by 16 threads in a fixed order.
// With outA, one more workgroup (the last) writes the column sums of A itself, outA[m] = sum_k A[k][m] (m < M; the bias
// gradient of the read-out layer, A = dOut), in a fixed order too.
__global__ __launch_bounds__(1024) void k_thin_tn_reduce(int N, int M, int S, const float *part, float *outW, int rows_w,
                                                         float *outB, const float *A, int lda, int K, float *outA) {
  __shared__ float red[16][64];
  if (outA && blockIdx.x == gridDim.x - 1) {
    float *r1 = &red[0][0];
    for (int m = 0; m < M; ++m) {
      float s = 0.f;
      for (int k = threadIdx.x; k < K; k += 1024) s += A[(size_t)k * lda + m];
      r1[threadIdx.x] = s;
      __syncthreads();
      for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) r1[threadIdx.x] += r1[threadIdx.x + h];
        __syncthreads();
      }
      if (threadIdx.x == 0) outA[m] = r1[0];
      __syncthreads();
    }
    return;
  }
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + c;
  const int total = (M + 1) * N;
  float s = 0.f;
  if (i < total)
    for (int z = q; z < S; z += 16) s += part[(size_t)z * total + i];
  red[q][c] = s;
  __syncthreads();
  if (q != 0 || i >= total) return;
  s = 0.f;
#pragma unroll
  for (int z = 0; z < 16; ++z) s += red[z][c];
  const int m = i / N;
  if (m < M) {
    if (outW && m < rows_w) outW[i] = s;
  } else if (outB) {
    outB[i - M * N] = s;
  }
}

// The read-out layer's backward in one pass over H2 (out_dim <= 8): dZ2 as k_dz2 writes it, and - from the same registers -
// the partials of dWf = dOut^T H2m (rows m < M of the thin product: H2 already holds relu(Z2) * mask) and of db2 = the
// column sums of dZ2 (row M), in k_thin_tn_part's layout and summation order: k_thin_tn_reduce finishes both.  Replaces
// thin product + k_dz2 + column sums (five launches) by two.
__global__ __launch_bounds__(256) void k_dz2_sums(int K, int N, int M, const float *__restrict__ dOut, const float *__restrict__ Wf,
                                                  const float *__restrict__ mask, const float *__restrict__ H2, float *__restrict__ dZ2,
                                                  float *__restrict__ part, int rows_per_block) {
  __shared__ float4 red[3][9][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = (blockIdx.x * 64 + lane) * 4;
  const bool col_ok = n < N;
  const int k0 = blockIdx.y * rows_per_block, k1 = min(K, k0 + rows_per_block);
  float4 acc[9], wf[8];
#pragma unroll
  for (int m = 0; m < 9; ++m) acc[m] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int m = 0; m < 8; ++m) wf[m] = (m < M && col_ok) ? *reinterpret_cast<const float4 *>(Wf + (size_t)m * N + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (col_ok)
    for (int k = k0 + wave; k < k1; k += 4) {
      const float4 h = *reinterpret_cast<const float4 *>(H2 + (size_t)k * N + n);
      const float *a = dOut + (size_t)k * M;  // wave-uniform: scalar loads
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int m = 0; m < 8; ++m)
        if (m < M) {
          const float am = a[m];
          s.x += am * wf[m].x; s.y += am * wf[m].y; s.z += am * wf[m].z; s.w += am * wf[m].w;
          acc[m].x += am * h.x; acc[m].y += am * h.y; acc[m].z += am * h.z; acc[m].w += am * h.w;
        }
      float4 g = make_float4(h.x > 0.f ? 1.f : 0.f, h.y > 0.f ? 1.f : 0.f, h.z > 0.f ? 1.f : 0.f, h.w > 0.f ? 1.f : 0.f);
      if (mask) {
        const float4 mk = *reinterpret_cast<const float4 *>(mask + (size_t)k * N + n);
        g.x *= mk.x; g.y *= mk.y; g.z *= mk.z; g.w *= mk.w;
      }
      const float4 dz = make_float4(s.x * g.x, s.y * g.y, s.z * g.z, s.w * g.w);
      *reinterpret_cast<float4 *>(dZ2 + (size_t)k * N + n) = dz;
      acc[8].x += dz.x; acc[8].y += dz.y; acc[8].z += dz.z; acc[8].w += dz.w;
    }
  thin_part_finish(acc, red, M, N, n, col_ok, part);
}

// read-out layers of up to this many outputs are served by the one-pass kernels below (k_linear_out, k_dz2_sums / k_dz2: H2 is
// read once, HBM-bound); wider ones (the critic: 100) by the matrix-core products with the epilogues EPI 2 / 3
constexpr int kThinOut = 8;
// out[n][o] = sum_c H2m[n][c] Wf[o][c] + bf[o]    (Linear 1000 -> out_dim); one wave per (node, o-chunk)
__global__ __launch_bounds__(256) void k_linear_out(int N, int hidden, int out_dim, const float *H2m, const float *Wf, const float *bf,
                                                    float *out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;
  if ((reinterpret_cast<uintptr_t>(Wf) | reinterpret_cast<uintptr_t>(H2m)) & 15) {  // (the C ABI takes any Wf: one column per lane)
    for (int o = 0; o < out_dim; ++o) {
      float s = 0.f;
      for (int c = lane; c < hidden; c += 64) s += H2m[(size_t)n * hidden + c] * Wf[(size_t)o * hidden + c];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
      if (lane == 0) out[(size_t)n * out_dim + o] = s + bf[o];
    }
    return;
  }
  const float4 *h = reinterpret_cast<const float4 *>(H2m + (size_t)n * hidden);
  const int h4 = hidden >> 2;
  for (int o = 0; o < out_dim; ++o) {
    const float4 *w = reinterpret_cast<const float4 *>(Wf + (size_t)o * hidden);
    float s = 0.f;
    for (int c = lane; c < h4; c += 64) {
      const float4 a = h[c], b = w[c];
      s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) out[(size_t)n * out_dim + o] = s + bf[o];
  }
}

// dZ2[n][c] = (sum_o dOut[n][o] Wf[o][c]) * mask[n][c] * (H2m > 0 <=> pre-activation > 0 and mask != 0)
// H2 holds relu(Z2) * mask, so "active" = (H2 != 0) when mask is a dropout mask of {0, 1/(1-p)}; the relu gate
// is recovered from H2 itself: Z2 > 0 and mask > 0  <=>  H2 > 0.
__global__ __launch_bounds__(256) void k_dz2(int N, int hidden, int out_dim, const float *dOut, const float *Wf, const float *mask,
                                             const float *H2, float *dZ2) {
  const int n = blockIdx.x;
  const uintptr_t al = reinterpret_cast<uintptr_t>(Wf) | reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(H2) | reinterpret_cast<uintptr_t>(dZ2);
  if ((hidden & 3) == 0 && (al & 15) == 0) {  // four columns per lane, 16-byte accesses
    for (int c4 = threadIdx.x; c4 < (hidden >> 2); c4 += 256) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int o = 0; o < out_dim; ++o) {
        const float d = dOut[(size_t)n * out_dim + o];
        const float4 w = reinterpret_cast<const float4 *>(Wf + (size_t)o * hidden)[c4];
        s.x += d * w.x; s.y += d * w.y; s.z += d * w.z; s.w += d * w.w;
      }
      const float4 h = reinterpret_cast<const float4 *>(H2 + (size_t)n * hidden)[c4];
      float4 g = make_float4(h.x > 0.f ? 1.f : 0.f, h.y > 0.f ? 1.f : 0.f, h.z > 0.f ? 1.f : 0.f, h.w > 0.f ? 1.f : 0.f);
      if (mask) {
        const float4 m = reinterpret_cast<const float4 *>(mask + (size_t)n * hidden)[c4];
        g.x *= m.x; g.y *= m.y; g.z *= m.z; g.w *= m.w;
      }
      reinterpret_cast<float4 *>(dZ2 + (size_t)n * hidden)[c4] = make_float4(s.x * g.x, s.y * g.y, s.z * g.z, s.w * g.w);
    }
    return;
  }
  for (int c = threadIdx.x; c < hidden; c += 256) {
    float s = 0.f;
    for (int o = 0; o < out_dim; ++o) s += dOut[(size_t)n * out_dim + o] * Wf[(size_t)o * hidden + c];
    const float h = H2[(size_t)n * hidden + c];
    float g = h > 0.f ? 1.f : 0.f;
    if (mask) g *= mask[(size_t)n * hidden + c];
    dZ2[(size_t)n * hidden + c] = s * g;
  }
}

// column sums (bias gradients): out[c] = sum_n X[n][c]; two deterministic stages
__global__ __launch_bounds__(256) void k_colsum_part(int N, int C, const float *X, float *part, int rows_per_block) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(N, r0 + rows_per_block);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += X[(size_t)r * C + c];
  part[(size_t)blockIdx.y * C + c] = s;
}

// K-slices of k_thin_tn_part / k_dz2_sums for K rows and `rows` output rows of N: up to 128 slices of at least 8 rows whose
// partials fit part_floats; returns the slice count, rows per slice in rpb
int thin_slices(int K, size_t rows, int N, size_t part_floats, int &rpb) {
  int nb = std::min(128, (K + 7) / 8);
  nb = (int)std::max<size_t>(1, std::min<size_t>(nb, part_floats / (rows * N)));
  rpb = (K + nb - 1) / nb;
  return (K + rpb - 1) / rpb;
}

// outW[rows_w x N] = (A^T B)[:rows_w], outB[N] = column sums of B, for M <= 8 columns of A (M = 0: column sums
// only): one pass over B. N % 4 == 0 and 16-byte aligned B rows (hidden-sized operands).
void thin_tn(hipStream_t st, float *part, size_t part_floats, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
             float *outW, int rows_w, float *outB, float *outA = nullptr) {
  int rpb;
  const int nb = thin_slices(K, (size_t)M + 1, N, part_floats, rpb);
  hipLaunchKernelGGL(k_thin_tn_part, dim3((N / 4 + 63) / 64, nb), dim3(256), 0, st, K, N, M, A, lda, B, ldb, part, rpb);
  hipLaunchKernelGGL(k_thin_tn_reduce, dim3(((M + 1) * N + 63) / 64 + (outA ? 1 : 0)), dim3(1024), 0, st, N, M, nb, part, outW, rows_w, outB,
                     A, lda, K, outA);
}

void colsum(hipStream_t st, float *part, size_t part_floats, int N, int C, const float *X, float *out) {
  if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0) {
    thin_tn(st, part, part_floats, 0, C, N, nullptr, 0, X, C, nullptr, 0, out);
    return;
  }
  const int nb = 64, rpb = (N + nb - 1) / nb;
  hipLaunchKernelGGL(k_colsum_part, dim3((C + 255) / 256, nb), dim3(256), 0, st, N, C, X, part, rpb);
  hipLaunchKernelGGL(k_splitk_reduce, dim3((C + 255) / 256), dim3(256), 0, st, C, nb, part, out);
}

}  // namespace
