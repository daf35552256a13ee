// g-U-Net policy network on gfx950: forward and backward of the graph U-Net trunk (scripts/Networks.py:125-449 over PyG 1.x
// GraphUNet: GCNConv(improved=True) everywhere, TopKPooling, sum_res, relu)
//   x_0 = relu(conv_d0(x, A_0));
//   level l = 1..depth:  B = offdiag((A_{l-1} + I)^2),  s = tanh(x_{l-1} . p_l / |p_l|),  perm_l = per graph the k = ceil(ratio n_g)
//     nodes of largest s (ties: lower index), kept in ascending index,  A_l = B[perm_l, perm_l] relabelled,
//     x_l = relu(conv_dl(x_{l-1}[perm_l] * s[perm_l], A_l));
//   i = 0..depth-1, j = depth-1-i:  x = conv_ui(x_j + up, A_j) with up[perm_{j+1}] = x, relu (the last one: the trunk's relu and the
//     dropout mask);  out = x Wf^T + bf.
// Matrix convention M[edge_index[0][e], edge_index[1][e]] = edge_attr[e], duplicates sum; edge weights are data (no gradient).
//
// Built over the parts of the GCN (k_gemm.hip, k_gcn_csr.hip, k_gcn_agg.hip, k_gcn_thin.hip), none of them edited: every conv is
// Â (input) through k_ax / k_aggregate over the CSRs the GCN's own builders make of the level's edge list, then the product with
// the fused bias + relu (+ mask) epilogue.  New here:
//   * k_unet_offsets: node offsets and edge capacities of every level (n_g <- ceil(ratio n_g) needs no scores);
//   * k_unet_pool: score, selection and gated gather of one graph per workgroup; the selection (unet_select, also alone as
//     k_unet_topk) ranks by counting over LDS tiles of the scores and compacts in index order with wave prefix sums: no sort,
//     no atomics;
//   * k_unet_augment: the product (A + I)^2 of one graph per workgroup, one thread per KEPT row with dense accumulators over the
//     graph's local columns in LDS, filtered to kept x kept and relabelled in the same pass - the unfiltered B never exists in
//     memory.  Output: the level's edge list sorted by (row, column) at the graph's capacity offset k_g (k_g - 1), unused slots
//     marked -1 (the GCN's builders ignore such edges);
//   * k_unet_unpool / k_unet_unpool_bwd (x_j + up in one pass; its backward a gather with the relu gate), k_unet_gate_bwd
//     (d x, d s through the tanh gate and the score's own path to x), k_unet_dp (d p_l with the term through |p|).
// fp32 throughout; every reduction in a fixed order: two runs are bit-equal.
#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>

#include "k_gemm.hip"
#include "k_gcn_csr.hip"
#include "k_gcn_agg.hip"
#include "k_gcn_thin.hip"

namespace {

constexpr int kUnetMaxDepth = 4;
constexpr int kUnetMaxGraphNodes = 4096;   // k_unet_augment keeps two dense rows of the graph per thread in LDS
constexpr int kUnetLdsWords = 32 * 1024;   // its LDS budget (128 KB)
constexpr int kUnetTile = 1024;            // scores per LDS tile of the selection
constexpr int kMetaInts = 32;              // per level: [0..4] nodes, [8..12] edge slots, [16..20] largest graph, [24..28] most slots of a graph

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }

// nodes kept of a graph of n: ceil(ratio n) in double, at least one, at most n (PyG TopKPooling)
__host__ __device__ inline int unet_keep(int n, double ratio) {
  if (n <= 0) return 0;
  const int k = (int)ceil(ratio * (double)n);
  return k < 1 ? 1 : (k > n ? n : k);
}

// ------------------------------------------------------------------------------------------------
// Offsets of every level: thread l walks the graphs once.  noff[l][g] = first node of graph g at level l, eoff[l][g] = first
// edge slot (level 0: the caller's edge_off; level l >= 1: the capacity prefix of k_g (k_g - 1)); rows are Gs + 1 apart.
// node_off = null: one graph of N nodes and E edges.  Levels first .. depth are written.  meta: the totals, the largest graph and
// the most edge slots of a graph per level (a capacity beyond INT_MAX is reported as INT_MAX).
// ------------------------------------------------------------------------------------------------
__global__ void k_unet_offsets(int Gs, int N, int E, const int *node_off, const int *edge_off, double ratio, int first, int depth, int *noff,
                               int *eoff, int *meta) {
  const int l = first + threadIdx.x;  // row threadIdx.x of noff / eoff
  if (l > depth) return;
  int *no = noff + (size_t)threadIdx.x * (Gs + 1), *eo = eoff ? eoff + (size_t)threadIdx.x * (Gs + 1) : nullptr;
  long long nsum = 0, esum = 0;
  int mx = 0, mxe = 0;
  for (int g = 0; g < Gs; ++g) {
    int n = node_off ? node_off[g + 1] - node_off[g] : N;
    if (n < 0) n = 0;
    for (int t = 0; t < l; ++t) n = unet_keep(n, ratio);
    const long long slots = l == 0 ? (edge_off ? max(edge_off[g + 1] - edge_off[g], 0) : E) : (long long)n * (n - 1);
    no[g] = (int)min(nsum, (long long)INT_MAX);
    if (eo) eo[g] = l == 0 ? (edge_off ? edge_off[g] : 0) : (int)min(esum, (long long)INT_MAX);
    nsum += n;
    esum += slots;
    mx = max(mx, n);
    mxe = (int)max((long long)mxe, min(slots, (long long)INT_MAX));
  }
  no[Gs] = (int)min(nsum, (long long)INT_MAX);
  if (eo) eo[Gs] = l == 0 ? (edge_off ? edge_off[Gs] : E) : (int)min(esum, (long long)INT_MAX);
  if (meta) {
    meta[l] = (int)min(nsum, (long long)INT_MAX);
    meta[8 + l] = (int)min(esum, (long long)INT_MAX);
    meta[16 + l] = mx;
    meta[24 + l] = mxe;
  }
}

// pn = p / |p|, inv[0] = 1 / |p|  (one workgroup; the sum of squares in a fixed order)
__global__ __launch_bounds__(256) void k_unet_pnorm(int C, const float *p, float *pn, float *inv) {
  __shared__ float red[256];
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) s += p[c] * p[c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const float iv = red[0] > 0.f ? 1.0f / sqrtf(red[0]) : 0.f;
  for (int c = threadIdx.x; c < C; c += 256) pn[c] = p[c] * iv;
  if (threadIdx.x == 0) inv[0] = iv;
}

// ------------------------------------------------------------------------------------------------
// Selection of one graph by its workgroup (256 threads): node i of the graph (scores sc[0 .. ng)) has rank = the number of the
// graph's nodes that beat it (larger score, or the same score and a lower index), counted over LDS tiles of the scores; it is
// kept while rank < k.  Kept nodes are compacted in index order: per chunk of 256 nodes a ballot per wave, the lanes below in the
// wave, the waves below in the chunk, the chunks before.  perm[m0 + pos] = n0 + i; inv[n0 + i] = m0 + pos or -1.
// (pos < k guards the stores: scores that do not order - NaN - must not overrun the graph's k slots.)
// ------------------------------------------------------------------------------------------------
__device__ void unet_select(const float *sc, int n0, int ng, int m0, int k, int *perm, int *inv, float *s_tile, int *s_wcnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int run = 0;
  for (int base = 0; base < ng; base += 256) {
    const int i = base + tid;
    const bool active = i < ng;
    const float si = active ? sc[i] : 0.f;
    int rank = 0;
    for (int t0 = 0; t0 < ng; t0 += kUnetTile) {
      const int tn = min(kUnetTile, ng - t0);
      __syncthreads();
      for (int j = tid; j < tn; j += 256) s_tile[j] = sc[t0 + j];
      __syncthreads();
      if (active)
        for (int j = 0; j < tn; ++j) {
          const float sj = s_tile[j];
          rank += (sj > si || (sj == si && t0 + j < i)) ? 1 : 0;
        }
    }
    const bool keep = active && rank < k;
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = run;
    for (int w = 0; w < wave; ++w) off += s_wcnt[w];
    const int pos = off + before;
    if (keep && pos < k) perm[m0 + pos] = n0 + i;
    if (active && inv) inv[n0 + i] = (keep && pos < k) ? m0 + pos : -1;
    run += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    __syncthreads();
  }
}

// the selection alone, from given scores (drlgx_unet_topk)
__global__ __launch_bounds__(256) void k_unet_topk(const float *scores, const int *noff_in, const int *noff_out, int *perm, int *inv) {
  __shared__ float s_tile[kUnetTile];
  __shared__ int s_wcnt[4];
  const int g = blockIdx.x;
  const int n0 = noff_in[g], ng = noff_in[g + 1] - n0, m0 = noff_out[g], k = noff_out[g + 1] - m0;
  unet_select(scores + n0, n0, ng, m0, k, perm, inv, s_tile, s_wcnt);
}

// Score, selection and gated gather of one graph: z = x . pn (one wave per node), s = tanh(z) -> S, Z; the selection over S;
// P[m] = x[perm[m]] * s[perm[m]] for the kept nodes, in their pooled order.
__global__ __launch_bounds__(256) void k_unet_pool(int C, const float *__restrict__ X, const float *__restrict__ pn, const int *noff_in,
                                                   const int *noff_out, float *S, float *Z, int *perm, int *inv, float *__restrict__ P) {
  __shared__ float s_tile[kUnetTile];
  __shared__ int s_wcnt[4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = noff_in[g], ng = noff_in[g + 1] - n0, m0 = noff_out[g], k = noff_out[g + 1] - m0;
  const int c4n = C >> 2;
  for (int i = wave; i < ng; i += 4) {
    const float *xr = X + (size_t)(n0 + i) * C;
    float d = 0.f;
    for (int c4 = lane; c4 < c4n; c4 += 64) {
      const float4 a = ld4(xr + 4 * c4), b = ld4(pn + 4 * c4);
      d += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off);
    if (lane == 0) {
      Z[n0 + i] = d;
      S[n0 + i] = tanhf(d);
    }
  }
  __threadfence_block();  // S of the whole graph is read below
  __syncthreads();
  unet_select(S + n0, n0, ng, m0, k, perm, inv, s_tile, s_wcnt);
  __threadfence_block();
  __syncthreads();
  for (int m = wave; m < k; m += 4) {
    const int n = perm[m0 + m];
    const float s = S[n];
    const float *xr = X + (size_t)n * C;
    float *pr = P + (size_t)(m0 + m) * C;
    for (int c4 = lane; c4 < c4n; c4 += 64) {
      const float4 a = ld4(xr + 4 * c4);
      st4(pr + 4 * c4, make_float4(a.x * s, a.y * s, a.z * s, a.w * s));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Augment and filter of one graph per workgroup: B = offdiag((A + I)^2) restricted to the kept nodes, relabelled.
// Thread t owns kept row i = perm[r0 + t] (T rows in flight; T from the LDS budget and the graph's size) with two dense vectors
// over the graph's ng local columns and a structural bit mask for each, interleaved by thread (word q of thread t at q T + t):
//   r[k]   = (A + I)[i][k]:  one scan of the graph's edges in edge order, then the 1 of the self loop;
//   acc[j] = sum over the edges e = (k -> j), in edge order, of r[k] w_e, then r[j] (the I of the right factor).
// Every thread walks the edges in the same order (wave-uniform loads).  Kept off-diagonal structural entries are counted, the
// rows' counts scanned over the workgroup in row order, and each thread writes its row's entries in column order: the output is
// sorted by (row, column), deterministic, and an entry is written once.  Edges with an endpoint outside the graph (the -1 of an
// unused slot among them) are ignored.  Slots [count, capacity) of the graph are marked -1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unet_augment(int lds_words, const int64_t *ei_in, size_t in_stride, const float *ew_in, const int *noff_in,
                                                      const int *eoff_in, const int *perm, const int *noff_out, const int *eoff_out,
                                                      int64_t *ei_out, size_t out_stride, float *ew_out, int *cnt_out) {
  extern __shared__ uint32_t s_aug[];
  __shared__ int s_w[4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = noff_in[g], ng = noff_in[g + 1] - n0, e0 = eoff_in[g], eg = eoff_in[g + 1] - e0;
  const int m0 = noff_out[g], k = noff_out[g + 1] - m0, o0 = eoff_out[g], ocap = eoff_out[g + 1] - o0;
  const int nw = (ng + 31) >> 5, per_row = 2 * ng + 2 * nw;
  int *s_new = reinterpret_cast<int *>(s_aug);  // [ng]: pooled local index of a local node, or -1
  uint32_t *rows = s_aug + ng;
  const int T = per_row > 0 ? min(256, (lds_words - ng) / per_row) : 0;
  int run = 0;
  if (T >= 1 && ng <= kUnetMaxGraphNodes) {
    for (int i = tid; i < ng; i += 256) s_new[i] = -1;
    __syncthreads();
    for (int m = tid; m < k; m += 256) {
      const int i = perm[m0 + m] - n0;
      if (i >= 0 && i < ng) s_new[i] = m;
    }
    __syncthreads();
    float *rf = reinterpret_cast<float *>(rows);
    const int R = 0, A = ng, RM = 2 * ng, AM = 2 * ng + nw;  // word offsets of r, acc and the two masks in a thread's slots
#define SLOT(q) ((size_t)(q) * T + tid)
    for (int r0 = 0; r0 < k; r0 += T) {
      const int m = r0 + tid;
      const bool act = tid < T && m < k;
      int i = act ? perm[m0 + m] - n0 : -1;
      const bool ok = act && i >= 0 && i < ng;
      if (tid < T)
        for (int q = 0; q < per_row; ++q) rows[SLOT(q)] = 0u;
      for (int e = 0; e < eg; ++e) {
        const long long a = ei_in[(size_t)e0 + e] - n0, b = ei_in[in_stride + e0 + e] - n0;
        if (a < 0 || a >= ng || b < 0 || b >= ng) continue;
        if (ok && (int)a == i) {
          rf[SLOT(R + (int)b)] += ew_in[e0 + e];
          rows[SLOT(RM + ((int)b >> 5))] |= 1u << ((int)b & 31);
        }
      }
      if (ok) {
        rf[SLOT(R + i)] += 1.0f;
        rows[SLOT(RM + (i >> 5))] |= 1u << (i & 31);
      }
      for (int e = 0; e < eg; ++e) {
        const long long a = ei_in[(size_t)e0 + e] - n0, b = ei_in[in_stride + e0 + e] - n0;
        if (a < 0 || a >= ng || b < 0 || b >= ng) continue;
        if (ok && ((rows[SLOT(RM + ((int)a >> 5))] >> ((int)a & 31)) & 1u)) {
          rf[SLOT(A + (int)b)] += rf[SLOT(R + (int)a)] * ew_in[e0 + e];
          rows[SLOT(AM + ((int)b >> 5))] |= 1u << ((int)b & 31);
        }
      }
      int cnt = 0;
      if (ok)
        for (int j = 0; j < ng; ++j) {
          if ((rows[SLOT(RM + (j >> 5))] >> (j & 31)) & 1u) {
            rf[SLOT(A + j)] += rf[SLOT(R + j)];
            rows[SLOT(AM + (j >> 5))] |= 1u << (j & 31);
          }
          cnt += (j != i && ((rows[SLOT(AM + (j >> 5))] >> (j & 31)) & 1u) && s_new[j] >= 0) ? 1 : 0;
        }
      // exclusive scan of the rows' counts over the workgroup, in row order
      int inc = cnt;
      for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
      }
      if (lane == 63) s_w[wave] = inc;
      __syncthreads();
      int pos = run + inc - cnt;
      for (int w = 0; w < wave; ++w) pos += s_w[w];
      if (ok)
        for (int j = 0; j < ng; ++j)
          if (j != i && ((rows[SLOT(AM + (j >> 5))] >> (j & 31)) & 1u) && s_new[j] >= 0) {
            if (pos < ocap) {
              ei_out[(size_t)o0 + pos] = m0 + m;
              ei_out[out_stride + o0 + pos] = m0 + s_new[j];
              ew_out[o0 + pos] = rf[SLOT(A + j)];
            }
            ++pos;
          }
      run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
      __syncthreads();
    }
#undef SLOT
  }
  run = min(run, ocap);
  for (int q = run + tid; q < ocap; q += 256) {
    ei_out[(size_t)o0 + q] = -1;
    ei_out[out_stride + o0 + q] = -1;
    ew_out[o0 + q] = 0.f;
  }
  if (tid == 0 && cnt_out) cnt_out[g] = run;
}

// ------------------------------------------------------------------------------------------------
// level 0's conv: X0 = relu(AX W + b) with AX = Â x (8 floats per node), a thread keeps its four W columns over kConvRows nodes
// ------------------------------------------------------------------------------------------------
constexpr int kConvRows = 16;
__global__ __launch_bounds__(256) void k_unet_conv0(int N, int in_dim, int hidden, const float *AX, const float *W, const float *b, float *out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= (hidden >> 2)) return;
  float4 w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = k < in_dim ? reinterpret_cast<const float4 *>(W + (size_t)k * hidden)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 bias = reinterpret_cast<const float4 *>(b)[c];
  const int r0 = blockIdx.y * kConvRows, r1 = min(N, r0 + kConvRows);
  for (int n = r0; n < r1; ++n) {
    const float4 v = h1_row(AX + (size_t)n * 8, in_dim, w, bias);
    reinterpret_cast<float4 *>(out + (size_t)n * hidden)[c] = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
  }
}

// U[n] = Xj[n] + (inv[n] >= 0 ? x[inv[n]] : 0): the unpool scatter and the residual sum in one pass, one thread per float4
__global__ __launch_bounds__(256) void k_unet_unpool(int N, int hidden, const float *__restrict__ Xj, const int *__restrict__ inv,
                                                     const float *__restrict__ x, float *__restrict__ U) {
  const int h4 = hidden >> 2;
  const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= (size_t)N * h4) return;
  const int n = (int)(item / h4), c = 4 * (int)(item - (size_t)n * h4);
  float4 v = ld4(Xj + (size_t)n * hidden + c);
  const int m = inv[n];
  if (m >= 0) {
    const float4 u = ld4(x + (size_t)m * hidden + c);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  st4(U + (size_t)n * hidden + c, v);
}
// its backward towards x: dx[m] = dU[perm[m]] * (y[m] > 0), y = the relu output that was unpooled
__global__ __launch_bounds__(256) void k_unet_unpool_bwd(int M, int hidden, const float *__restrict__ dU, const int *__restrict__ perm,
                                                         const float *__restrict__ y, float *__restrict__ dx) {
  const int h4 = hidden >> 2;
  const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= (size_t)M * h4) return;
  const int m = (int)(item / h4), c = 4 * (int)(item - (size_t)m * h4);
  const float4 d = ld4(dU + (size_t)perm[m] * hidden + c), yv = ld4(y + (size_t)m * hidden + c);
  st4(dx + (size_t)m * hidden + c, make_float4(yv.x > 0.f ? d.x : 0.f, yv.y > 0.f ? d.y : 0.f, yv.z > 0.f ? d.z : 0.f, yv.w > 0.f ? d.w : 0.f));
}

// ------------------------------------------------------------------------------------------------
// Backward of the gate, one workgroup per node n of the level above the pool (x = x_{l-1}, relu output):
//   kept (m = inv[n] >= 0):  ds = dP[m] . x[n],  dz = ds (1 - s^2) -> dzf[n],
//                            dZ[n] = (res[n] + dP[m] s + dz pn) * (x[n] > 0)       (pn = p / |p|: the score's own path to x)
//   dropped:                 dZ[n] = res[n] * (x[n] > 0),  dzf[n] = 0               (the selection is discrete)
// res = the gradient that reached x_{l-1} along the residual of the up path.  The dot product: per-thread partial, shuffle
// reduction per wave, the four waves' sums added in a fixed order.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unet_gate_bwd(int hidden, const float *__restrict__ x, const int *__restrict__ inv,
                                                       const float *__restrict__ dP, const float *__restrict__ S, const float *__restrict__ pn,
                                                       const float *__restrict__ res, float *__restrict__ dZ, float *__restrict__ dzf) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h4 = hidden >> 2;
  const int m = inv[n];
  const float *xr = x + (size_t)n * hidden, *rr = res + (size_t)n * hidden;
  float *zr = dZ + (size_t)n * hidden;
  if (m < 0) {
    for (int c4 = tid; c4 < h4; c4 += 256) {
      const float4 xv = ld4(xr + 4 * c4), r = ld4(rr + 4 * c4);
      st4(zr + 4 * c4, make_float4(xv.x > 0.f ? r.x : 0.f, xv.y > 0.f ? r.y : 0.f, xv.z > 0.f ? r.z : 0.f, xv.w > 0.f ? r.w : 0.f));
    }
    if (tid == 0) dzf[n] = 0.f;
    return;
  }
  const float *dr = dP + (size_t)m * hidden;
  float d = 0.f;
  for (int c4 = tid; c4 < h4; c4 += 256) {
    const float4 a = ld4(dr + 4 * c4), b = ld4(xr + 4 * c4);
    d += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  }
  for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off);
  if (lane == 0) red[wave] = d;
  __syncthreads();
  const float ds = ((red[0] + red[1]) + red[2]) + red[3];
  const float s = S[n], dz = ds * (1.f - s * s);
  if (tid == 0) dzf[n] = dz;
  for (int c4 = tid; c4 < h4; c4 += 256) {
    const float4 a = ld4(dr + 4 * c4), xv = ld4(xr + 4 * c4), r = ld4(rr + 4 * c4), q = ld4(pn + 4 * c4);
    float4 o = make_float4(r.x + a.x * s + dz * q.x, r.y + a.y * s + dz * q.y, r.z + a.z * s + dz * q.z, r.w + a.w * s + dz * q.w);
    o.x = xv.x > 0.f ? o.x : 0.f; o.y = xv.y > 0.f ? o.y : 0.f; o.z = xv.z > 0.f ? o.z : 0.f; o.w = xv.w > 0.f ? o.w : 0.f;
    st4(zr + 4 * c4, o);
  }
}

// d p[c] = (t[c] - q pn[c]) / |p|  with t = dzf^T x (the thin product before this) and q = sum_n dzf[n] z[n] (z = x . p / |p|):
// d z / d p = (x - z p / |p|) / |p|.  q by every workgroup in the same fixed order.
__global__ __launch_bounds__(256) void k_unet_dp(int C, int N, const float *t, const float *dzf, const float *Z, const float *pn, const float *inv,
                                                 float *dp) {
  __shared__ float red[256];
  float s = 0.f;
  for (int n = threadIdx.x; n < N; n += 256) s += dzf[n] * Z[n];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const float q = red[0];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) dp[c] = (t[c] - q * pn[c]) * inv[0];
}

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
struct UnetCsr {  // what k_ax / k_aggregate read of one level, as the GCN's builders write it
  float *deg, *selfw, *wn_dst, *wn_src;
  int *ptr_dst, *end_dst, *ptr_src, *end_src, *nbr_dst, *nbr_src;
};
struct UnetLevel {
  UnetCsr csr;
  int64_t *EI;            // level >= 1: the pooled edge list [2][Ecap] (level 0: the caller's)
  float *EW;
  float *X, *AH;          // the down conv's relu output and its aggregated input (level 0: AH = AX, 8 floats per node)
  float *AHU, *Y;         // level < depth: the up conv's aggregated input (the backward reuses it for d(x_j + up)) and relu output
  float *S, *Z, *DZF, *PN, *INV;  // level >= 1: scores, pre-tanh scores and d z over the nodes of level - 1; p / |p|, 1 / |p|
  int *perm, *inv;        // level >= 1: kept nodes (ids of level - 1) [N_l]; pooled id or -1 [N_{l-1}]
};
struct UnetWs {
  int *meta, *noff, *eoff;
  UnetLevel lv[kUnetMaxDepth + 1];
  float *T0, *T1, *T2, *TP, *part;
  int *cnt_dst, *cnt_src, *cur_dst, *cur_src, *eid_dst, *eid_src;
  size_t part_floats, counters_bytes;
};
struct UnetBounds {  // host-side upper bounds of the levels' sizes
  size_t N[kUnetMaxDepth + 1], E[kUnetMaxDepth + 1];
  int kmax[kUnetMaxDepth + 1];
  bool ok;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

UnetBounds unet_bounds(int n_nodes, int n_edges, int n_graphs, int max_graph_nodes, int depth, double ratio) {
  UnetBounds b;
  const int Gs = std::max(n_graphs, 1);
  b.ok = max_graph_nodes >= 1 && max_graph_nodes <= kUnetMaxGraphNodes;
  b.N[0] = (size_t)n_nodes;
  b.E[0] = (size_t)std::max(n_edges, 1);
  b.kmax[0] = std::min(max_graph_nodes, n_nodes);
  for (int l = 1; l <= depth; ++l) {
    // sum of ceil(ratio n_g) <= ratio N + G; a graph keeps at most kmax nodes, hence at most kmax (kmax - 1) entries
    b.N[l] = std::max<size_t>(1, std::min<size_t>(b.N[l - 1], (size_t)std::floor(ratio * (double)b.N[l - 1]) + Gs + 1));
    b.kmax[l] = unet_keep(b.kmax[l - 1], ratio);
    b.E[l] = std::max<size_t>(1, b.N[l] * (size_t)std::max(b.kmax[l] - 1, 0));
    if (b.E[l] > (size_t)INT_MAX / 4) b.ok = false;
  }
  return b;
}

// lays the workspace out from `base` (null: for its size only) by the bounds and returns its bytes
size_t carve(UnetWs &w, char *base, const UnetBounds &b, int n_graphs, int hidden, int depth) {
  size_t off = 0;
  auto take = [&](auto *&p, size_t n) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
    off += align256(n * sizeof(*p));
  };
  const int Gs = std::max(n_graphs, 1);
  const size_t C = hidden;
  take(w.meta, kMetaInts);
  take(w.noff, (size_t)(depth + 1) * (Gs + 1));
  take(w.eoff, (size_t)(depth + 1) * (Gs + 1));
  size_t Emax = 1;
  for (int l = 0; l <= depth; ++l) {
    UnetLevel &y = w.lv[l];
    const size_t N = b.N[l], E = b.E[l];
    Emax = std::max(Emax, E);
    take(y.csr.deg, N);
    take(y.csr.selfw, N);
    take(y.csr.wn_dst, E);
    take(y.csr.wn_src, E);
    take(y.csr.ptr_dst, N + 1);
    take(y.csr.end_dst, N + 1);
    take(y.csr.ptr_src, N + 1);
    take(y.csr.end_src, N + 1);
    take(y.csr.nbr_dst, E);
    take(y.csr.nbr_src, E);
    take(y.X, N * C);
    take(y.AH, l == 0 ? N * 8 : N * C);
    if (l < depth) {
      take(y.AHU, N * C);
      take(y.Y, N * C);
    } else {
      y.AHU = y.Y = nullptr;
    }
    if (l >= 1) {
      take(y.EI, 2 * E);
      take(y.EW, E);
      take(y.S, b.N[l - 1]);
      take(y.Z, b.N[l - 1]);
      take(y.DZF, b.N[l - 1]);
      take(y.PN, C);
      take(y.INV, 1);
      take(y.perm, N);
      take(y.inv, b.N[l - 1]);
    } else {
      y.EI = nullptr;
      y.EW = y.S = y.Z = y.DZF = y.PN = y.INV = nullptr;
      y.perm = y.inv = nullptr;
    }
  }
  const size_t N0C = b.N[0] * C;
  take(w.T0, N0C);
  take(w.T1, N0C);
  take(w.T2, N0C);
  take(w.TP, C);
  // split-K partials of a hidden x hidden gradient (8 slices), the thin products' (up to 9 rows, 128 slices)
  const size_t part = std::max<size_t>((size_t)8 * C * C, (size_t)128 * 9 * C);
  take(w.part, part);
  w.part_floats = part;
  const size_t Nmax = b.N[0];
  take(w.cnt_dst, Nmax + 1);  // the four counters are contiguous: one memset
  take(w.cnt_src, Nmax + 1);
  take(w.cur_dst, Nmax + 1);
  take(w.cur_src, Nmax + 1);
  w.counters_bytes = off - ((char *)w.cnt_dst - base);
  take(w.eid_dst, Emax);
  take(w.eid_src, Emax);
  return off;
}

dim3 panel_grid(size_t N, int hidden) { return dim3((unsigned)((N * (size_t)(hidden >> 2) + 255) / 256)); }

// normalisation and both CSRs of one level's edge list (E slots, unused ones -1): the GCN's one-launch build per graph when the
// graphs' slot ranges fit its sort, else its generic count / scan / fill / sort / finish sequence.  AX = Â x for level 0.
void build_level(hipStream_t st, const UnetWs &w, const UnetCsr &c, int N, int E, const int64_t *ei, const float *ew, int G, const int *noff,
                 const int *eoff, int max_slots_per_graph, const float *x, int in_dim, float *AX) {
  const drlgx_csr_cache rows = {c.deg, c.selfw, AX, c.ptr_dst, c.end_dst, c.ptr_src, c.end_src, c.nbr_dst, c.nbr_src, c.wn_dst, c.wn_src};
  if (G > 0 && launch_csr_graphs(st, G, noff, eoff, max_slots_per_graph, N, E, ei, ew, x, in_dim, rows, 0)) return;
  hipMemsetAsync(w.cnt_dst, 0, w.counters_bytes, st);
  hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.selfw), 0x40000000, (size_t)N, st);  // 2.0f: the improved-GCN fill value
  if (E > 0) hipLaunchKernelGGL(k_degree, dim3((E + 255) / 256), dim3(256), 0, st, N, E, ei, ew, w.cnt_dst, w.cnt_src, c.selfw);
  hipLaunchKernelGGL(k_scan2, dim3(1), dim3(1024), 0, st, N, w.cnt_dst, c.ptr_dst, w.cnt_src, c.ptr_src);
  if (E > 0)
    hipLaunchKernelGGL(k_csr_fill, dim3((E + 255) / 256), dim3(256), 0, st, N, E, ei, c.ptr_dst, w.cur_dst, w.eid_dst, c.ptr_src, w.cur_src, w.eid_src);
  const dim3 gn((N + 127) / 128), g2((2 * N + 127) / 128), bn(128);
  hipLaunchKernelGGL(k_csr_sort, g2, bn, 0, st, N, c.ptr_dst, w.eid_dst, c.ptr_src, w.eid_src);
  hipLaunchKernelGGL(k_degree_sum, gn, bn, 0, st, N, ew, c.ptr_src, w.eid_src, c.selfw, c.deg);
  hipLaunchKernelGGL(k_csr_finish, g2, bn, 0, st, N, E, ei, ew, c.deg, c.ptr_dst, w.eid_dst, c.nbr_dst, c.wn_dst, c.ptr_src, w.eid_src, c.nbr_src,
                     c.wn_src, c.end_dst, c.end_src);
  if (AX)
    hipLaunchKernelGGL(k_ax, dim3((N * 8 + 255) / 256), dim3(256), 0, st, N, in_dim, x, c.deg, c.selfw, c.ptr_dst, c.end_dst, c.nbr_dst, c.wn_dst, AX);
}

void launch_augment(hipStream_t st, int G, int max_nodes, int max_kept, const int64_t *ei_in, size_t in_stride, const float *ew_in, const int *noff_in,
                    const int *eoff_in, const int *perm, const int *noff_out, const int *eoff_out, int64_t *ei_out, size_t out_stride,
                    float *ew_out, int *cnt_out) {
  const int nw = (max_nodes + 31) >> 5;
  // as many rows in flight as the largest graph keeps, while they fit
  const size_t want = (size_t)max_nodes + (size_t)std::min(256, std::max(max_kept, 1)) * (2 * (size_t)max_nodes + 2 * nw);
  const int lds_words = (int)std::min<size_t>(kUnetLdsWords, std::max<size_t>(want, 64));
  static bool attr_set[32] = {false};
  const void *fns[] = {reinterpret_cast<const void *>(&k_unet_augment)};
  drlgx_ensure_lds_attr(attr_set, fns, 1, kUnetLdsWords * 4);
  hipLaunchKernelGGL(k_unet_augment, dim3(G), dim3(256), (size_t)lds_words * 4, st, lds_words, ei_in, in_stride, ew_in, noff_in, eoff_in, perm,
                     noff_out, eoff_out, ei_out, out_stride, ew_out, cnt_out);
}

bool unet_args_ok(int n_nodes, int n_edges, int n_graphs, int max_graph_nodes, int in_dim, int hidden, int depth, double ratio, int out_dim) {
  return n_nodes > 0 && n_edges >= 0 && n_graphs >= 0 && max_graph_nodes >= 1 && in_dim > 0 && in_dim <= 8 && hidden > 0 && !(hidden & 3) &&
         depth >= 1 && depth <= kUnetMaxDepth && ratio > 0.0 && ratio <= 1.0 && out_dim > 0;
}

// the levels' exact sizes, read back from the workspace (the forward's k_unet_offsets left them there)
struct UnetSizes {
  int N[kUnetMaxDepth + 1], E[kUnetMaxDepth + 1], mx[kUnetMaxDepth + 1], mxe[kUnetMaxDepth + 1];
};
int read_sizes(hipStream_t st, const UnetWs &w, const UnetBounds &b, int n_nodes, int depth, UnetSizes &s) {
  int meta[kMetaInts];
  if (hipMemcpyAsync(meta, w.meta, sizeof(meta), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return DRLGX_E_HIP;
  for (int l = 0; l <= depth; ++l) {
    s.N[l] = meta[l];
    s.E[l] = meta[8 + l];
    s.mx[l] = meta[16 + l];
    s.mxe[l] = meta[24 + l];
  }
  if (s.N[0] != n_nodes) return DRLGX_E_INVALID;  // node_off does not cover the nodes
  if (s.mx[0] > b.kmax[0]) return DRLGX_E_CAPACITY;  // a graph larger than the caller's bound: the workspace was sized for less
  for (int l = 0; l <= depth; ++l)
    if (s.N[l] < 1 || (size_t)s.N[l] > b.N[l] || (l >= 1 && (size_t)s.E[l] > b.E[l]) || (l == 0 && (size_t)s.E[0] > b.E[0])) return DRLGX_E_CAPACITY;
  return DRLGX_OK;
}

}  // namespace

extern "C" {

size_t drlgx_unet_workspace_bytes(int n_nodes, int n_edges, int n_graphs, int max_graph_nodes, int hidden, int depth, double pool_ratio, int out_dim) {
  if (!unet_args_ok(n_nodes, n_edges, n_graphs, max_graph_nodes, 1, hidden, depth, pool_ratio, out_dim)) return 0;
  const UnetBounds b = unet_bounds(n_nodes, n_edges, n_graphs, max_graph_nodes, depth, pool_ratio);
  if (!b.ok) return 0;
  UnetWs sizing;
  return carve(sizing, nullptr, b, n_graphs, hidden, depth) + 256;
}

int drlgx_unet_topk(void *hip_stream, int n_nodes, int n_graphs, const int32_t *node_off, const float *scores, double pool_ratio,
                    int32_t *pooled_node_off, int32_t *pooled_edge_off, int32_t *perm, int32_t *inverse) {
  if (n_nodes <= 0 || n_graphs <= 0 || !node_off || !scores || !(pool_ratio > 0.0 && pool_ratio <= 1.0) || !pooled_node_off || !perm)
    return DRLGX_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL(k_unet_offsets, dim3(1), dim3(64), 0, st, n_graphs, n_nodes, 0, node_off, (const int *)nullptr, pool_ratio, 1, 1, pooled_node_off,
                     pooled_edge_off, (int *)nullptr);
  hipLaunchKernelGGL(k_unet_topk, dim3(n_graphs), dim3(256), 0, st, scores, node_off, pooled_node_off, perm, inverse);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_unet_augment_filter(void *hip_stream, int n_nodes, int n_edges, const int64_t *edge_index, const float *edge_attr, int n_graphs,
                              const int32_t *node_off, const int32_t *edge_off, int max_graph_nodes, const int32_t *perm,
                              const int32_t *pooled_node_off, const int32_t *pooled_edge_off, int64_t pooled_capacity, int64_t *pooled_edge_index,
                              float *pooled_edge_attr, int32_t *pooled_edge_count) {
  if (n_nodes <= 0 || n_edges < 0 || n_graphs <= 0 || !node_off || !edge_off || !perm || !pooled_node_off || !pooled_edge_off ||
      pooled_capacity < 0 || (pooled_capacity > 0 && (!pooled_edge_index || !pooled_edge_attr)) || (n_edges > 0 && (!edge_index || !edge_attr)) ||
      max_graph_nodes < 1)
    return DRLGX_E_INVALID;
  if (max_graph_nodes > kUnetMaxGraphNodes) return DRLGX_E_CAPACITY;
  launch_augment(reinterpret_cast<hipStream_t>(hip_stream), n_graphs, max_graph_nodes, max_graph_nodes, edge_index, (size_t)n_edges, edge_attr, node_off, edge_off, perm,
                 pooled_node_off, pooled_edge_off, pooled_edge_index, (size_t)pooled_capacity, pooled_edge_attr, pooled_edge_count);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_unet_forward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int depth, double pool_ratio, int out_dim, const float *x,
                       const int64_t *edge_index, const float *edge_attr, const float *const *params, const float *dropout_mask, float *out,
                       void *ws_dev, size_t ws_bytes, int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_graph_nodes) {
  if (!unet_args_ok(n_nodes, n_edges, n_graphs, max_graph_nodes, in_dim, hidden, depth, pool_ratio, out_dim) || !x || !params || !out || !ws_dev ||
      (n_edges > 0 && (!edge_index || !edge_attr)) || (n_graphs > 0 && (!node_off || !edge_off)))
    return DRLGX_E_INVALID;
  const int n_params = 4 * depth + 4 + depth;
  uintptr_t al = reinterpret_cast<uintptr_t>(dropout_mask);
  for (int i = 0; i < n_params; ++i) {
    if (!params[i]) return DRLGX_E_INVALID;
    al |= reinterpret_cast<uintptr_t>(params[i]);
  }
  if (al & 15) return DRLGX_E_INVALID;  // (weights, biases, pool vectors and the mask are read by 16-byte loads)
  const UnetBounds b = unet_bounds(n_nodes, n_edges, n_graphs, max_graph_nodes, depth, pool_ratio);
  if (!b.ok) return DRLGX_E_CAPACITY;
  UnetWs w;
  if (carve(w, reinterpret_cast<char *>(ws_dev), b, n_graphs, hidden, depth) > ws_bytes) return DRLGX_E_CAPACITY;  // nothing written
  // state_dict order: down_convs.{0..depth}.{weight,bias}, pools.{0..depth-1}.weight, up_convs.{0..depth-1}.{weight,bias}, fully_con1
  const float *const *down = params, *const *pool = params + 2 * (depth + 1), *const *up = pool + depth;
  const float *Wf = up[2 * depth], *bf = up[2 * depth + 1];
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int C = hidden, Gs = std::max(n_graphs, 1);
  const dim3 b256(256);
  hipLaunchKernelGGL(k_unet_offsets, dim3(1), dim3(64), 0, st, Gs, n_nodes, n_edges, n_graphs > 0 ? node_off : nullptr,
                     n_graphs > 0 ? edge_off : nullptr, pool_ratio, 0, depth, w.noff, w.eoff, w.meta);
  UnetSizes z;
  if (const int rc = read_sizes(st, w, b, n_nodes, depth, z)) return rc;
  auto noff = [&](int l) { return w.noff + (size_t)l * (Gs + 1); };
  auto eoff = [&](int l) { return w.eoff + (size_t)l * (Gs + 1); };
  // level 0: x_0 = relu(Â x W + b)
  {
    const UnetLevel &y = w.lv[0];
    build_level(st, w, y.csr, n_nodes, n_edges, edge_index, edge_attr, n_graphs, node_off, edge_off, z.mxe[0], x, in_dim, y.AH);
    hipLaunchKernelGGL(k_unet_conv0, dim3(((C >> 2) + 255) / 256, (n_nodes + kConvRows - 1) / kConvRows), b256, 0, st, n_nodes, in_dim, C, y.AH, down[0],
                       down[1], y.X);
  }
  for (int l = 1; l <= depth; ++l) {
    const UnetLevel &y = w.lv[l], &a = w.lv[l - 1];
    const int N = z.N[l];
    hipLaunchKernelGGL(k_unet_pnorm, dim3(1), b256, 0, st, C, pool[l - 1], y.PN, y.INV);
    hipLaunchKernelGGL(k_unet_pool, dim3(Gs), b256, 0, st, C, a.X, y.PN, noff(l - 1), noff(l), y.S, y.Z, y.perm, y.inv, w.T0);
    const int64_t *ei_in = l == 1 ? edge_index : a.EI;
    // the pooled edge list is [2][z.E[l]]: the slots in use are known on the host, and the GCN's builders read row 1 at + E
    const size_t in_stride = l == 1 ? (size_t)n_edges : (size_t)z.E[l - 1];
    launch_augment(st, Gs, z.mx[l - 1], z.mx[l], ei_in, in_stride, l == 1 ? edge_attr : a.EW, noff(l - 1), eoff(l - 1), y.perm, noff(l), eoff(l), y.EI,
                   (size_t)z.E[l], y.EW, nullptr);
    build_level(st, w, y.csr, N, z.E[l], y.EI, y.EW, z.E[l] > 0 ? Gs : 0, noff(l), eoff(l), z.mxe[l], nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_aggregate<false>, dim3(N), b256, 0, st, N, C, w.T0, y.csr.deg, y.csr.selfw, y.csr.ptr_dst, y.csr.end_dst, y.csr.nbr_dst,
                       y.csr.wn_dst, 0, nullptr, nullptr, nullptr, y.AH);
    gemm<false, false, 1>(st, N, C, C, y.AH, C, down[2 * l], C, y.X, C, down[2 * l + 1], nullptr, 1);
  }
  const float *xc = w.lv[depth].X;
  for (int i = 0; i < depth; ++i) {
    const int j = depth - 1 - i;
    const UnetLevel &y = w.lv[j];
    const int N = z.N[j];
    hipLaunchKernelGGL(k_unet_unpool, panel_grid(N, C), b256, 0, st, N, C, y.X, w.lv[j + 1].inv, xc, w.T0);
    hipLaunchKernelGGL(k_aggregate<false>, dim3(N), b256, 0, st, N, C, w.T0, y.csr.deg, y.csr.selfw, y.csr.ptr_dst, y.csr.end_dst, y.csr.nbr_dst,
                       y.csr.wn_dst, 0, nullptr, nullptr, nullptr, y.AHU);
    // relu after every up conv: the last one's is the trunk's own relu, with the dropout mask
    gemm<false, false, 1>(st, N, C, C, y.AHU, C, up[2 * i], C, y.Y, C, up[2 * i + 1], i == depth - 1 ? dropout_mask : nullptr, 1);
    xc = y.Y;
  }
  if (out_dim <= kThinOut)
    hipLaunchKernelGGL(k_linear_out, dim3((n_nodes + 3) / 4), b256, 0, st, n_nodes, C, out_dim, xc, Wf, bf, out);
  else
    gemm<false, true, 2>(st, n_nodes, out_dim, C, xc, C, Wf, C, out, out_dim, bf, nullptr, 1);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_unet_backward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int depth, double pool_ratio, int out_dim, const float *x,
                        const int64_t *edge_index, const float *edge_attr, const float *const *params, const float *dropout_mask,
                        const float *d_out, float *const *grads, void *ws_dev, size_t ws_bytes, int n_graphs, int max_graph_nodes) {
  if (!unet_args_ok(n_nodes, n_edges, n_graphs, max_graph_nodes, in_dim, hidden, depth, pool_ratio, out_dim) || !params || !d_out || !grads || !ws_dev)
    return DRLGX_E_INVALID;
  const int n_params = 4 * depth + 4 + depth;
  for (int i = 0; i < n_params; ++i)
    if (!params[i] || !grads[i]) return DRLGX_E_INVALID;
  (void)x; (void)edge_index; (void)edge_attr;  // the forward left every level's CSRs, panels, scores and kept sets in ws
  const UnetBounds b = unet_bounds(n_nodes, n_edges, n_graphs, max_graph_nodes, depth, pool_ratio);
  if (!b.ok) return DRLGX_E_CAPACITY;
  UnetWs w;
  if (carve(w, reinterpret_cast<char *>(ws_dev), b, n_graphs, hidden, depth) > ws_bytes) return DRLGX_E_CAPACITY;
  const float *const *down = params, *const *up = params + 2 * (depth + 1) + depth;
  float *const *d_down = grads, *const *d_pool = grads + 2 * (depth + 1), *const *d_up = d_pool + depth;
  const float *Wf = up[2 * depth];
  float *dWf = d_up[2 * depth], *dbf = d_up[2 * depth + 1];
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int C = hidden;
  const dim3 b256(256);
  UnetSizes z;
  if (const int rc = read_sizes(st, w, b, n_nodes, depth, z)) return rc;
  // read-out layer: T0 = d(last up conv's pre-activation) = (dOut Wf) * (Y > 0) * mask, as the GCN's dZ2 (Y plays H2)
  const float *Yl = w.lv[0].Y;
  float *db_last = d_up[2 * (depth - 1) + 1];
  const uintptr_t al16 = reinterpret_cast<uintptr_t>(Wf) | reinterpret_cast<uintptr_t>(dropout_mask);
  bool db_last_done = false;
  if (out_dim <= kThinOut && (al16 & 15) == 0) {
    int rpb;
    const int nb = thin_slices(n_nodes, (size_t)out_dim + 1, C, w.part_floats, rpb);
    hipLaunchKernelGGL(k_dz2_sums, dim3((C / 4 + 63) / 64, nb), b256, 0, st, n_nodes, C, out_dim, d_out, Wf, dropout_mask, Yl, w.T0, w.part, rpb);
    hipLaunchKernelGGL(k_thin_tn_reduce, dim3(((out_dim + 1) * C + 63) / 64 + 1), dim3(1024), 0, st, C, out_dim, nb, w.part, dWf, out_dim, db_last,
                       d_out, out_dim, n_nodes, dbf);
    db_last_done = true;
  } else if (out_dim <= kThinOut) {
    thin_tn(st, w.part, w.part_floats, out_dim, C, n_nodes, d_out, out_dim, Yl, C, dWf, out_dim, nullptr, dbf);
    hipLaunchKernelGGL(k_dz2, dim3(n_nodes), b256, 0, st, n_nodes, C, out_dim, d_out, Wf, dropout_mask, Yl, w.T0);
  } else {
    gemm_tn_splitk(st, w.part, w.part_floats, out_dim, C, n_nodes, d_out, out_dim, Yl, C, dWf, 32);
    colsum(st, w.part, w.part_floats, n_nodes, out_dim, d_out, dbf);
    gemm<false, false, 3>(st, n_nodes, C, out_dim, d_out, out_dim, Wf, C, w.T0, C, Yl, dropout_mask, 1);
  }
  // up path, last conv first: T0 holds dZ of up conv i at level j
  for (int i = depth - 1; i >= 0; --i) {
    const int j = depth - 1 - i;
    const UnetLevel &y = w.lv[j];
    const int N = z.N[j], Nn = z.N[j + 1];
    gemm_tn_splitk(st, w.part, w.part_floats, C, C, N, y.AHU, C, w.T0, C, d_up[2 * i]);  // dW = (Â U)^T dZ
    if (!(db_last_done && i == depth - 1)) colsum(st, w.part, w.part_floats, N, C, w.T0, d_up[2 * i + 1]);
    gemm<false, true, 0>(st, N, C, C, w.T0, C, up[2 * i], C, w.T1, C, nullptr, nullptr, 1);  // T1 = dZ W^T
    hipLaunchKernelGGL(k_aggregate<false>, dim3(N), b256, 0, st, N, C, w.T1, y.csr.deg, y.csr.selfw, y.csr.ptr_src, y.csr.end_src, y.csr.nbr_src,
                       y.csr.wn_src, 0, nullptr, nullptr, nullptr, y.AHU);  // AHU <- d(x_j + up) = Â^T T1: the residual's share stays here
    const float *prev = i == 0 ? w.lv[depth].X : w.lv[j + 1].Y;  // what was unpooled into this conv's input
    hipLaunchKernelGGL(k_unet_unpool_bwd, panel_grid(Nn, C), b256, 0, st, Nn, C, y.AHU, w.lv[j + 1].perm, prev, w.T0);
  }
  // down path: T0 holds dZ of down conv l
  for (int l = depth; l >= 1; --l) {
    const UnetLevel &y = w.lv[l], &a = w.lv[l - 1];
    const int N = z.N[l], Np = z.N[l - 1];
    gemm_tn_splitk(st, w.part, w.part_floats, C, C, N, y.AH, C, w.T0, C, d_down[2 * l]);
    colsum(st, w.part, w.part_floats, N, C, w.T0, d_down[2 * l + 1]);
    gemm<false, true, 0>(st, N, C, C, w.T0, C, down[2 * l], C, w.T1, C, nullptr, nullptr, 1);
    hipLaunchKernelGGL(k_aggregate<false>, dim3(N), b256, 0, st, N, C, w.T1, y.csr.deg, y.csr.selfw, y.csr.ptr_src, y.csr.end_src, y.csr.nbr_src,
                       y.csr.wn_src, 0, nullptr, nullptr, nullptr, w.T2);  // T2 = d(x_{l-1}[perm] * s[perm])
    hipLaunchKernelGGL(k_unet_gate_bwd, dim3(Np), b256, 0, st, C, a.X, y.inv, w.T2, y.S, y.PN, a.AHU, w.T0, y.DZF);
    thin_tn(st, w.part, w.part_floats, 1, C, Np, y.DZF, 1, a.X, C, w.TP, 1, nullptr);  // TP = dzf^T x_{l-1}
    hipLaunchKernelGGL(k_unet_dp, dim3((C + 255) / 256), b256, 0, st, C, Np, w.TP, y.DZF, y.Z, y.PN, y.INV, d_pool[l - 1]);
  }
  // level 0: dW = AX^T dZ (AX rows are 8 wide), db = colsum(dZ)
  thin_tn(st, w.part, w.part_floats, 8, C, n_nodes, w.lv[0].AH, 8, w.T0, C, d_down[0], in_dim, d_down[1]);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_unet_kept_nodes(void *hip_stream, int n_nodes, int n_edges, int hidden, int depth, double pool_ratio, int out_dim, void *ws_dev,
                          size_t ws_bytes, int n_graphs, int max_graph_nodes, int level, int32_t *perm_out, int *count_host) {
  if (!unet_args_ok(n_nodes, n_edges, n_graphs, max_graph_nodes, 1, hidden, depth, pool_ratio, out_dim) || !ws_dev || level < 1 || level > depth ||
      !perm_out || !count_host)
    return DRLGX_E_INVALID;
  const UnetBounds b = unet_bounds(n_nodes, n_edges, n_graphs, max_graph_nodes, depth, pool_ratio);
  if (!b.ok) return DRLGX_E_CAPACITY;
  UnetWs w;
  if (carve(w, reinterpret_cast<char *>(ws_dev), b, n_graphs, hidden, depth) > ws_bytes) return DRLGX_E_CAPACITY;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  UnetSizes z;
  if (const int rc = read_sizes(st, w, b, n_nodes, depth, z)) return rc;
  if (hipMemcpyAsync(perm_out, w.lv[level].perm, (size_t)z.N[level] * sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess) return DRLGX_E_HIP;
  *count_host = z.N[level];
  return DRLGX_OK;
}

}  // extern "C"
