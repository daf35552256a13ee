// The aggregations Â H of the GCN over the CSRs of k_gcn_csr.hip.
#pragma once
#include "drlgx_dev.h"

namespace {

// ------------------------------------------------------------------------------------------------
// layer 1 and the aggregation of layer 2, without materialising H1:
//   AX = Â X (in_dim <= 8 features, rows padded to 8)                                     k_ax, one thread per (node, k)
//   AH1[n] = sum_i w_i relu(AX[m_i] W1 + b1)  over n itself (self weight) and its neighbours   k_aggregate_l1
// A row of H1 = relu(AX[m] W1 + b1) costs in_dim FMAs per element from 32 bytes of AX, against 4 KB of HBM / L2 traffic to
// write it once and gather it ~8 times: it is recomputed where it is needed (also as the ReLU gate of the backward pass),
// in the same operation order as a stored H1 would have had.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ax(int N, int in_dim, const float *x, const float *deg, const float *selfw, const int *ptr,
                                            const int *pend, const int *nbr, const float *wn, float *AX) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n = e >> 3, t = e & 7;
  if (n >= N) return;
  float s = 0.f;
  if (t < in_dim) {
    s = (selfw[n] / deg[n]) * x[(size_t)n * in_dim + t];  // self loop: dis * w_self * dis
    for (int i = ptr[n]; i < pend[n]; ++i) s += wn[i] * x[(size_t)nbr[i] * in_dim + t];
  }
  AX[(size_t)n * 8 + t] = s;
}

// H1[m][4c .. 4c+3] from AX[m] (8 floats), this thread's four W1 columns (w[k]) and biases: one FMA chain over k per column,
// written on two-float vectors so that it compiles to v_pk_fma_f32 (two columns per instruction, a[k] broadcast).  Left to
// itself the compiler packs along k instead - v_pk_mul_f32 + two v_add_f32 per pair of products, 28 VALU instructions per
// (row, four columns) where 10 + 4 (ReLU) + 2 (weighted sum) do.
typedef float floatx2 __attribute__((ext_vector_type(2)));
template <int IN>
__device__ __forceinline__ void h1_core(floatx2 &lo, floatx2 &hi, const float (&a)[8], int in_dim, const float4 (&w)[8], const float4 &bias) {
  lo = floatx2{bias.x, bias.y};
  hi = floatx2{bias.z, bias.w};
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (IN > 0 ? k < IN : k < in_dim) {
      const floatx2 ak = {a[k], a[k]};
      lo = __builtin_elementwise_fma(ak, floatx2{w[k].x, w[k].y}, lo);
      hi = __builtin_elementwise_fma(ak, floatx2{w[k].z, w[k].w}, hi);
    }
}
// ... from the row's 8 AX values at ax (in memory, or staged in LDS); IN > 0: the number of input features at compile time (the
// reference's 5): straight-line code
template <int IN = 0>
__device__ __forceinline__ float4 h1_row(const float *ax, int in_dim, const float4 (&w)[8], const float4 &bias) {
  const float4 a0 = reinterpret_cast<const float4 *>(ax)[0], a1 = reinterpret_cast<const float4 *>(ax)[1];
  const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  floatx2 lo, hi;
  h1_core<IN>(lo, hi, a, in_dim, w, bias);
  return make_float4(lo.x, lo.y, hi.x, hi.y);  // pre-activation
}
// acc += wi * relu(u)
__device__ __forceinline__ void relu_axpy(floatx2 &alo, floatx2 &ahi, float wi, const float4 &u) {
  const floatx2 w2 = {wi, wi};
  alo = __builtin_elementwise_fma(w2, floatx2{fmaxf(u.x, 0.f), fmaxf(u.y, 0.f)}, alo);
  ahi = __builtin_elementwise_fma(w2, floatx2{fmaxf(u.z, 0.f), fmaxf(u.w, 0.f)}, ahi);
}

constexpr int kAggStage = 64;  // neighbour rows of AX (and their weights) staged in LDS; longer rows read the rest from memory
constexpr int kAggNodes = 4;   // nodes per workgroup: the thread's W1 columns and biases are loaded once for all of them, and
                               // the neighbour lists of all of them are staged together (one round of memory latency)
static_assert(kAggNodes * kAggStage == 256, "one staging thread per (node, neighbour slot)");
// Every memory access of the kernel sits in ONE dependent chain of three loads (row bounds -> neighbour id -> its AX row),
// walked once by every thread for its own (node, slot) with the W1 columns requested in front of it; the multiply loop
// reads LDS only.  (The first version staged 8 elements per thread in a loop - 24 dependent round trips - and loaded W1
// and the row bounds behind one wait each: 57 us for the 17 288-node batch, a fifth of the VALU rate.)
template <int IN>
__global__ __launch_bounds__(256) void k_aggregate_l1(int N, int in_dim, int hidden, const float *AX, const float *W1, const float *b1,
                                                      const float *deg, const float *selfw, const int *ptr, const int *pend, const int *nbr,
                                                      const float *wn, float *out, float *b1_keep) {
  __shared__ __attribute__((aligned(16))) float s_ax[kAggNodes][(kAggStage + 1) * 8];  // slot kAggStage: the node's own row
  __shared__ float s_wn[kAggNodes][kAggStage + 1];                                       // slot kAggStage: its self weight
  __shared__ int s_ab[kAggNodes][2];
  const int tid = threadIdx.x;
  const int h4 = hidden >> 2;
  const int nb0 = blockIdx.x * kAggNodes, nn = min(kAggNodes, N - nb0);
  auto load_w = [&](float4 (&w)[8], float4 &bias, int c) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      w[k] = (IN > 0 ? k < IN : k < in_dim) ? reinterpret_cast<const float4 *>(W1 + (size_t)k * hidden)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    bias = reinterpret_cast<const float4 *>(b1)[c];
  };
  float4 w[8], bias;
  load_w(w, bias, min(tid, h4 - 1));  // (unconditional: under a branch the compiler waits for the loads before leaving it)
  {
    // every load unconditional (clamped to a valid element), only the LDS stores are predicated: under branches the loads
    // of the own row / self weight / neighbour row would each be waited for in turn
    const int q = tid >> 6, j = tid & (kAggStage - 1), n = min(nb0 + q, N - 1);
    const float4 *AX4 = reinterpret_cast<const float4 *>(AX);
    const int a = ptr[n], b = pend[n];
    const float4 own = AX4[(size_t)n * 2 + (j & 1)];
    const float sw = selfw[n], dg = deg[n];
    const int e = max(min(a + j, b - 1), 0);
    const int m = a + j < b ? nbr[e] : n;  // (outside the row nbr[e] may be a never-written gap of the batched CSR: not an address)
    const float wv = wn[e];
    const float4 r0 = AX4[(size_t)m * 2], r1 = AX4[(size_t)m * 2 + 1];
    if (q < nn) {
      if (j < 2) reinterpret_cast<float4 *>(s_ax[q] + 8 * kAggStage)[j] = own;
      if (j == 2) {
        s_wn[q][kAggStage] = sw / dg;
        s_ab[q][0] = a;
        s_ab[q][1] = b;
      }
      if (a + j < b) {
        s_wn[q][j] = wv;
        reinterpret_cast<float4 *>(s_ax[q] + 8 * j)[0] = r0;
        reinterpret_cast<float4 *>(s_ax[q] + 8 * j)[1] = r1;
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < h4; c += 256) {
    if (c != tid) load_w(w, bias, c);
    if (blockIdx.x == 0) reinterpret_cast<float4 *>(b1_keep)[c] = bias;  // the backward pass's copy of b1 (the ReLU gate of layer 1)
    for (int q = 0; q < nn; ++q) {
      const int n = nb0 + q;
      const int a = s_ab[q][0], b = s_ab[q][1];
      const int ns = min(b - a, kAggStage);
      const float self = s_wn[q][kAggStage];
      const float4 v = h1_row<IN>(s_ax[q] + 8 * kAggStage, in_dim, w, bias);
      floatx2 alo = {self * fmaxf(v.x, 0.f), self * fmaxf(v.y, 0.f)}, ahi = {self * fmaxf(v.z, 0.f), self * fmaxf(v.w, 0.f)};
      for (int j = 0; j < ns; ++j) relu_axpy(alo, ahi, s_wn[q][j], h1_row<IN>(s_ax[q] + 8 * j, in_dim, w, bias));
      for (int i = a + ns; i < b; ++i) relu_axpy(alo, ahi, wn[i], h1_row<IN>(AX + (size_t)nbr[i] * 8, in_dim, w, bias));
      reinterpret_cast<float4 *>(out + (size_t)n * hidden)[c] = make_float4(alo.x, alo.y, ahi.x, ahi.y);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// aggregation out[n] = (selfw[n]/deg[n]) H[n] + sum_i wn[i] H[nbr[i]], optionally gated by H1[n] > 0 with H1 recomputed
// from AX / W1 / b1 (the ReLU of layer 1 in the backward pass);  one workgroup per node, float4 per lane
// ------------------------------------------------------------------------------------------------
template <bool kGate>
__global__ __launch_bounds__(256) void k_aggregate(int N, int hidden, const float *H, const float *deg, const float *selfw, const int *ptr,
                                                   const int *pend, const int *nbr, const float *wn, int in_dim, const float *AX,
                                                   const float *W1, const float *b1, float *out) {
  const int n = blockIdx.x;
  const int h4 = hidden >> 2;
  const float self = selfw[n] / deg[n];
  const int a = ptr[n], b = pend[n];
  for (int c = threadIdx.x; c < h4; c += 256) {
    float4 v = reinterpret_cast<const float4 *>(H + (size_t)n * hidden)[c];
    float4 acc = make_float4(self * v.x, self * v.y, self * v.z, self * v.w);
    for (int i = a; i < b; ++i) {
      const float w = wn[i];
      const float4 u = reinterpret_cast<const float4 *>(H + (size_t)nbr[i] * hidden)[c];
      acc.x += w * u.x; acc.y += w * u.y; acc.z += w * u.z; acc.w += w * u.w;
    }
    if (kGate) {
      float4 wk[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) wk[k] = k < in_dim ? reinterpret_cast<const float4 *>(W1 + (size_t)k * hidden)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 g = h1_row(AX + (size_t)n * 8, in_dim, wk, reinterpret_cast<const float4 *>(b1)[c]);
      acc.x = g.x > 0.f ? acc.x : 0.f; acc.y = g.y > 0.f ? acc.y : 0.f;
      acc.z = g.z > 0.f ? acc.z : 0.f; acc.w = g.w > 0.f ? acc.w : 0.f;
    }
    reinterpret_cast<float4 *>(out + (size_t)n * hidden)[c] = acc;
  }
}

}  // namespace
