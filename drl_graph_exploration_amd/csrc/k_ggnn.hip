// GG-NN policy network on gfx950: forward and backward of the gated graph trunk
//   h_0 = [x | 0];  per layer l:  a = (A h_l) W_l,  h_{l+1} = GRUCell(a, h_l);  Hm = relu(h_L) [* dropout mask],  out = Hm Wf^T + bf
// with (A h)[i] = sum over the edges e with edge_index[1][e] = i of edge_attr[e] h[edge_index[0][e]]: the plain weighted sum at the
// TARGET node, no self loops added, no normalisation (PyG 1.x GatedGraphConv(1000, 3), aggr = 'add'; scripts/Networks.py:73-122
// GGNN / PolicyGGNN / ValueGGNN trunks).  GRUCell as torch.nn.GRUCell, gate order r, z, n:
//   r = s(W_ir a + b_ir + W_hr h + b_hr),  z = s(W_iz a + b_iz + W_hz h + b_hz),  n = tanh(W_in a + b_in + r (W_hn h + b_hn)),
//   h' = (1 - z) n + z h.
//
// Built over the parts of the GCN (k_gemm.hip, k_gcn_csr.hip, k_gcn_agg.hip, k_gcn_thin.hip); new here are the GRU gate, forward
// and backward (k_gru_gate, k_gru_gate_bwd: LDS-free, one float4 of the features per thread, every panel touched once), the thin
// products of layer 0, the raw-weight finish of the CSRs and the one-launch raw-weight build of a batch of small graphs.
//   * raw weights: both CSRs carry edge_attr itself (k_csr_raw after the generic count / scan / fill / sort, or k_csr_graphs_raw),
//     deg = 1 and selfw = 0, so that k_ax and k_aggregate compute the plain sum.  (As in the GCN build an explicit self loop is not
//     a CSR entry but the node's self weight - one per node; the exploration graphs have none.)
//   * aggregate first, multiply second: (A h) W_l.  Layer 0 has in_dim <= 8 live columns: A h_0 is the 8-floats-per-node AX,
//     a = AX W_0[:in_dim] and W_hh h_0 are thin products (k_thin_nn, k_thin_nt), the gate reads x for h_0's live columns.
//   * gate pre-activations: gi = a W_ih^T and gh = h W_hh^T, N x hidden . hidden x 3 hidden on gemm<>.
//   * saved per layer for the backward: h_l, A h_l, a, and the gates r, z, n with hn = W_hn h + b_hn (four panels; the two
//     pre-activation panels would be six, and recomputing them two more GEMMs per layer).  gi / gh are temporaries; the backward
//     reuses them for d(gi) / d(gh).
//   * backward, per layer from the last: k_gru_gate_bwd (d(gi), d(gh), z dh'), the GRU's weight gradients per gate through
//     gemm_tn_splitk and its bias gradients through colsum, accumulated over the layers in a fixed order (k_acc); da = d(gi) W_ih,
//     d(A h) = da W_l^T, dweight[l] = (A h)^T da, dh = z dh' + d(gh) W_hh + A^T d(A h) (by-source CSR).  Layer 0 produces no dx;
//     rows >= in_dim of dweight[0] are zeros.
// fp32 throughout; every reduction in a fixed order: two runs are bit-equal.
#include <algorithm>

#include "k_gemm.hip"
#include "k_gcn_csr.hip"
#include "k_gcn_agg.hip"
#include "k_gcn_thin.hip"

namespace {

// ------------------------------------------------------------------------------------------------
// raw-weight finish of the generic CSR build: (neighbour, edge_attr) per slot of both CSRs, explicit row ends
// ------------------------------------------------------------------------------------------------
__global__ void k_csr_raw(int N, int E, const int64_t *ei, const float *ew, const int *ptr_dst, const int *eid_dst, int *nbr_dst, float *wn_dst,
                          const int *ptr_src, const int *eid_src, int *nbr_src, float *wn_src, int *end_dst, int *end_src, float *deg) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= 2 * N) return;
  const bool by_dst = n < N;
  const int *ptr = by_dst ? ptr_dst : ptr_src, *eid = by_dst ? eid_dst : eid_src;
  int *nbr = by_dst ? nbr_dst : nbr_src;
  float *wn = by_dst ? wn_dst : wn_src;
  if (!by_dst) n -= N;
  else deg[n] = 1.0f;
  (by_dst ? end_dst : end_src)[n] = ptr[n + 1];
  for (int i = ptr[n]; i < ptr[n + 1]; ++i) {
    const int e = eid[i];
    nbr[i] = (int)(by_dst ? ei[e] : ei[(size_t)E + e]);
    wn[i] = ew[e];
  }
}

// ------------------------------------------------------------------------------------------------
// Both raw-weight CSRs of a BATCH of small graphs in one launch, one workgroup per graph (graph g owns nodes [node_off[g],
// node_off[g+1]) and edges [edge_off[g], edge_off[g+1]); edges with an endpoint outside their graph are ignored, a self loop is
// the node's self weight - the rules of the generic build).  No sort: the slot of edge j in a CSR is its rank among the graph's
// edges by (row node, edge id), counted over the graph's edges in LDS - quadratic in the edge count, a few hundred per graph
// here; the launcher sends batches with larger graphs (> kRawMaxEdges) to the generic build.  Rows come out by node with their
// entries in edge order: the generic build's rows, bit for bit (rows packed from edge_off[g]; explicit row ends).
// ------------------------------------------------------------------------------------------------
constexpr int kRawMaxEdges = 2048;
constexpr int kRawNone = 0x7fffffff;  // row key of an ignored edge / a self loop: ranks behind every row

__global__ __launch_bounds__(256) void k_csr_graphs_raw(int E, const int64_t *ei, const float *ew, const int *node_off, const int *edge_off,
                                                        float *deg, float *selfw, int *ptr_dst, int *end_dst, int *nbr_dst, float *wn_dst,
                                                        int *ptr_src, int *end_src, int *nbr_src, float *wn_src) {
  __shared__ int s_src[kRawMaxEdges], s_dst[kRawMaxEdges];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = node_off[g], n1 = node_off[g + 1], e0 = edge_off[g];
  const int ng = n1 - n0, eg = min(edge_off[g + 1] - e0, kRawMaxEdges);  // (the caller promised eg <= kRawMaxEdges)
  for (int m = tid; m < ng; m += 256) {
    selfw[n0 + m] = 0.f;
    deg[n0 + m] = 1.f;
  }
  __syncthreads();  // (selfw: the zeros before the self loops' weights)
  for (int j = tid; j < eg; j += 256) {
    const int64_t r = ei[e0 + j], c = ei[(size_t)E + e0 + j];
    int a = kRawNone, b = kRawNone;
    if (r >= n0 && r < n1 && c >= n0 && c < n1) {
      if (r == c) {
        selfw[r] = ew[e0 + j];
      } else {
        a = (int)(r - n0);
        b = (int)(c - n0);
      }
    }
    s_src[j] = a;
    s_dst[j] = b;
  }
  __syncthreads();
  // rows: [edges of smaller row node, + edges of this one)
  for (int m = tid; m < ng; m += 256) {
    int ls = 0, cs = 0, ld = 0, cd = 0;
    for (int k = 0; k < eg; ++k) {
      const int a = s_src[k], b = s_dst[k];
      ls += a < m; cs += a == m;
      ld += b < m; cd += b == m;
    }
    ptr_src[n0 + m] = e0 + ls;
    end_src[n0 + m] = e0 + ls + cs;
    ptr_dst[n0 + m] = e0 + ld;
    end_dst[n0 + m] = e0 + ld + cd;
  }
  // entries: rank by (row node, edge id)
  for (int j = tid; j < eg; j += 256) {
    const int a = s_src[j], b = s_dst[j];
    if (a == kRawNone) continue;
    int ra = 0, rb = 0;
    for (int k = 0; k < eg; ++k) {
      const int ak = s_src[k], bk = s_dst[k];
      ra += ak < a || (ak == a && k < j);
      rb += bk < b || (bk == b && k < j);
    }
    const float w = ew[e0 + j];
    nbr_src[e0 + ra] = n0 + b;
    wn_src[e0 + ra] = w;
    nbr_dst[e0 + rb] = n0 + a;
    wn_dst[e0 + rb] = w;
  }
}

// ------------------------------------------------------------------------------------------------
// thin products of layer 0 (h_0 has in_dim <= 8 live columns)
//   k_thin_nn: out[n][c] = sum_k AX[n][k] W[k][c]            (a = (A x) W_0[:in_dim]; AX rows are 8 floats, zero from in_dim on)
//   k_thin_nt: out[n][j] = sum_k x[n][k] W[j][k], k < in_dim  (gh = h_0 W_hh^T over h_0's live columns; W rows are ldw apart)
// a thread keeps its weights in registers over kThinRows nodes
// ------------------------------------------------------------------------------------------------
constexpr int kThinRows = 16;
__global__ __launch_bounds__(256) void k_thin_nn(int N, int in_dim, int hidden, const float *AX, const float *W, float *out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= (hidden >> 2)) return;
  float4 w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = k < in_dim ? reinterpret_cast<const float4 *>(W + (size_t)k * hidden)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const int r0 = blockIdx.y * kThinRows, r1 = min(N, r0 + kThinRows);
  for (int n = r0; n < r1; ++n) reinterpret_cast<float4 *>(out + (size_t)n * hidden)[c] = h1_row(AX + (size_t)n * 8, in_dim, w, zero);
}
__global__ __launch_bounds__(256) void k_thin_nt(int N, int in_dim, int J, const float *x, const float *W, int ldw, float *out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= J) return;
  float w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = k < in_dim ? W[(size_t)j * ldw + k] : 0.f;
  const int r0 = blockIdx.y * kThinRows, r1 = min(N, r0 + kThinRows);
  for (int n = r0; n < r1; ++n) {
    const float *xr = x + (size_t)n * in_dim;  // wave-uniform: scalar loads
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < in_dim) s += xr[k] * w[k];
    out[(size_t)n * J + j] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// The GRU gate.  One thread per (node, four adjacent features); no LDS, no loop: the launch is as wide as the panel and the
// hardware's many short waves cover the HBM latency.  THIN: h is h_0 = [x | 0], read from x (in_dim floats per node).
// LAST: the trunk's relu and dropout mask are applied in the same pass and only the masked panel is written (the read-out
// layer reads it directly).
//   reads  gi, gh [N][3 hidden] (r | z | n pre-activations without their biases), h, b_ih, b_hh (, mask)
//   writes h' (or Hm), and the saved r, z, n, hn = gh_n + b_hn
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
// h_0[n][4 c4 .. + 3]
__device__ __forceinline__ float4 h0_quad(const float *x, int in_dim, int n, int c4) {
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = 4 * c4 + i < in_dim ? x[(size_t)n * in_dim + 4 * c4 + i] : 0.f;
  return make_float4(v[0], v[1], v[2], v[3]);
}

template <bool THIN, bool LAST>
__global__ __launch_bounds__(256) void k_gru_gate(int N, int hidden, int in_dim, const float *__restrict__ gi, const float *__restrict__ gh,
                                                  const float *__restrict__ h, const float *__restrict__ b_ih, const float *__restrict__ b_hh,
                                                  const float *__restrict__ mask, float *__restrict__ hout, float *__restrict__ R,
                                                  float *__restrict__ Z, float *__restrict__ Nn, float *__restrict__ HN) {
  const int h4 = hidden >> 2;
  const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= (size_t)N * h4) return;
  const int n = (int)(item / h4), c4 = (int)(item - (size_t)n * h4), c = 4 * c4;
  const size_t at = (size_t)n * hidden + c, at3 = (size_t)n * 3 * hidden + c;
  const float4 ir = ld4(gi + at3), iz = ld4(gi + at3 + hidden), in = ld4(gi + at3 + 2 * hidden);
  const float4 hr = ld4(gh + at3), hz = ld4(gh + at3 + hidden), hn = ld4(gh + at3 + 2 * hidden);
  const float4 bir = ld4(b_ih + c), biz = ld4(b_ih + hidden + c), bin = ld4(b_ih + 2 * hidden + c);
  const float4 bhr = ld4(b_hh + c), bhz = ld4(b_hh + hidden + c), bhn = ld4(b_hh + 2 * hidden + c);
  const float4 hv = THIN ? h0_quad(h, in_dim, n, c4) : ld4(h + at);
  float4 mk = make_float4(1.f, 1.f, 1.f, 1.f);
  if (LAST && mask) mk = ld4(mask + at);
  float4 r, z, nn, hnb, o;
#define DRLGX_GRU_LANE(f)                                   \
  r.f = sigmoidf_((ir.f + bir.f) + (hr.f + bhr.f));         \
  z.f = sigmoidf_((iz.f + biz.f) + (hz.f + bhz.f));         \
  hnb.f = hn.f + bhn.f;                                     \
  nn.f = tanhf((in.f + bin.f) + r.f * hnb.f);               \
  o.f = (1.f - z.f) * nn.f + z.f * hv.f;                    \
  if (LAST) o.f = fmaxf(o.f, 0.f) * mk.f;
  DRLGX_GRU_LANE(x) DRLGX_GRU_LANE(y) DRLGX_GRU_LANE(z) DRLGX_GRU_LANE(w)
#undef DRLGX_GRU_LANE
  st4(hout + at, o);
  st4(R + at, r);
  st4(Z + at, z);
  st4(Nn + at, nn);
  st4(HN + at, hnb);
}

// Backward of the gate: from dh' and the saved r, z, n, hn and h
//   d(gi) = (dr~, dz~, dn~),  d(gh) = (dr~, dz~, r dn~)  with  dn~ = dh' (1 - z) (1 - n^2),  dz~ = dh' (h - n) z (1 - z),
//   dr~ = dn~ hn r (1 - r);  dh_direct = z dh'  (not written when null: layer 0 has no dh)
template <bool THIN>
__global__ __launch_bounds__(256) void k_gru_gate_bwd(int N, int hidden, int in_dim, const float *__restrict__ dh, const float *__restrict__ h,
                                                      const float *__restrict__ R, const float *__restrict__ Z, const float *__restrict__ Nn,
                                                      const float *__restrict__ HN, float *__restrict__ dgi, float *__restrict__ dgh,
                                                      float *__restrict__ dh_direct) {
  const int h4 = hidden >> 2;
  const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= (size_t)N * h4) return;
  const int n = (int)(item / h4), c4 = (int)(item - (size_t)n * h4), c = 4 * c4;
  const size_t at = (size_t)n * hidden + c, at3 = (size_t)n * 3 * hidden + c;
  const float4 d = ld4(dh + at), r = ld4(R + at), z = ld4(Z + at), nn = ld4(Nn + at), hn = ld4(HN + at);
  const float4 hv = THIN ? h0_quad(h, in_dim, n, c4) : ld4(h + at);
  float4 dr, dz, dn, dnr, dd;
#define DRLGX_GRU_LANE(f)                                   \
  dn.f = d.f * (1.f - z.f) * (1.f - nn.f * nn.f);           \
  dz.f = d.f * (hv.f - nn.f) * (z.f * (1.f - z.f));         \
  dr.f = dn.f * hn.f * (r.f * (1.f - r.f));                 \
  dnr.f = dn.f * r.f;                                       \
  dd.f = d.f * z.f;
  DRLGX_GRU_LANE(x) DRLGX_GRU_LANE(y) DRLGX_GRU_LANE(z) DRLGX_GRU_LANE(w)
#undef DRLGX_GRU_LANE
  st4(dgi + at3, dr);
  st4(dgi + at3 + hidden, dz);
  st4(dgi + at3 + 2 * hidden, dn);
  st4(dgh + at3, dr);
  st4(dgh + at3 + hidden, dz);
  st4(dgh + at3 + 2 * hidden, dnr);
  if (dh_direct) st4(dh_direct + at, dd);
}

// acc[i] += t[i]  (the GRU's gradients summed over the layers, last layer first); acc[i] += t[i] + u[i] with u
__global__ void k_acc(size_t n, float *acc, const float *t, const float *u) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  acc[i] += u ? t[i] + u[i] : t[i];
}
// dW[j][k] += t[k][j], k < in_dim: layer 0's share of dW_hh (t = x^T d(gh), [in_dim][J]) into its first in_dim columns
__global__ void k_acc_t(int J, int in_dim, int ldw, float *dW, const float *t) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= J) return;
  for (int k = 0; k < in_dim; ++k) dW[(size_t)j * ldw + k] += t[(size_t)k * J + j];
}

// ------------------------------------------------------------------------------------------------
struct GgnnLayer {
  float *H, *AH, *A, *R, *Z, *Nn, *HN;  // H: the layer's input h_l (layer 0: null, it is x); AH: A h_l (layer 0: AX, 8 floats per node)
};
constexpr int kGgnnMaxLayers = 16;
struct GgnnWs {
  float *deg, *selfw, *wn_dst, *wn_src, *Hm, *GI, *GH, *D0, *D1, *DA, *T1, *T2, *T3, *TW, *TB, *part;
  GgnnLayer layer[kGgnnMaxLayers];
  int *cnt_dst, *cnt_src, *ptr_dst, *ptr_src, *cur_dst, *cur_src, *eid_dst, *eid_src, *nbr_dst, *nbr_src, *end_dst, *end_src;
  size_t part_floats, counters_bytes;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// lays the workspace out from `base` (null: for its size only, the pointers are then offsets) and returns its bytes
size_t carve(GgnnWs &w, char *base, int N, int E, int hidden, int L) {
  size_t off = 0;
  auto takef = [&](float *&p, size_t n) {
    p = reinterpret_cast<float *>(base + off);
    off += align256(n * sizeof(float));
  };
  auto takei = [&](int *&p, size_t n) {
    p = reinterpret_cast<int *>(base + off);
    off += align256(n * sizeof(int));
  };
  const size_t NH = (size_t)N * hidden;
  // split-K partials of a hidden x hidden gradient (8 slices), and the thin products' (up to 9 rows of 3 hidden, 128 slices)
  const size_t part = std::max<size_t>((size_t)8 * hidden * hidden, (size_t)128 * 9 * 3 * hidden);
  takef(w.deg, N);
  takef(w.selfw, N);
  takef(w.wn_dst, E);
  takef(w.wn_src, E);
  for (int l = 0; l < L; ++l) {
    GgnnLayer &y = w.layer[l];
    if (l == 0) {
      y.H = nullptr;
      takef(y.AH, (size_t)N * 8);
    } else {
      takef(y.H, NH);
      takef(y.AH, NH);
    }
    takef(y.A, NH);
    takef(y.R, NH);
    takef(y.Z, NH);
    takef(y.Nn, NH);
    takef(y.HN, NH);
  }
  takef(w.Hm, NH);
  takef(w.GI, 3 * NH);
  takef(w.GH, 3 * NH);
  takef(w.D0, NH);
  takef(w.D1, NH);
  takef(w.DA, NH);
  takef(w.T1, NH);
  takef(w.T2, NH);
  takef(w.T3, NH);
  takef(w.TW, std::max<size_t>((size_t)hidden * hidden, (size_t)8 * 3 * hidden));  // one gate's weight gradient of one layer, or layer 0's thin [in_dim][3 hidden]
  takef(w.TB, (size_t)3 * hidden);
  takef(w.part, part);
  w.part_floats = part;
  takei(w.cnt_dst, N + 1);  // the four counters are contiguous: one memset (see build_graph_raw)
  takei(w.cnt_src, N + 1);
  takei(w.cur_dst, N + 1);
  takei(w.cur_src, N + 1);
  w.counters_bytes = off - ((char *)w.cnt_dst - base);
  takei(w.ptr_dst, N + 1);
  takei(w.ptr_src, N + 1);
  takei(w.eid_dst, E);
  takei(w.eid_src, E);
  takei(w.nbr_dst, E);
  takei(w.nbr_src, E);
  takei(w.end_dst, N + 1);
  takei(w.end_src, N + 1);
  return off;
}

// both raw-weight CSRs of any edge list: the generic count / scan / fill / sort of k_gcn_csr.hip, then k_csr_raw
void build_graph_raw(hipStream_t st, const GgnnWs &w, int N, int E, const int64_t *ei, const float *ew) {
  hipMemsetAsync(w.cnt_dst, 0, w.counters_bytes, st);  // cnt_dst, cnt_src, cur_dst, cur_src
  hipMemsetAsync(w.selfw, 0, (size_t)N * sizeof(float), st);
  if (E > 0) {
    hipLaunchKernelGGL(k_degree, dim3((E + 255) / 256), dim3(256), 0, st, N, E, ei, ew, w.cnt_dst, w.cnt_src, w.selfw);
  }
  hipLaunchKernelGGL(k_scan2, dim3(1), dim3(1024), 0, st, N, w.cnt_dst, w.ptr_dst, w.cnt_src, w.ptr_src);
  if (E > 0) {
    hipLaunchKernelGGL(k_csr_fill, dim3((E + 255) / 256), dim3(256), 0, st, N, E, ei, w.ptr_dst, w.cur_dst, w.eid_dst, w.ptr_src,
                       w.cur_src, w.eid_src);
  }
  const dim3 g2((2 * N + 127) / 128), bn(128);
  hipLaunchKernelGGL(k_csr_sort, g2, bn, 0, st, N, w.ptr_dst, w.eid_dst, w.ptr_src, w.eid_src);
  hipLaunchKernelGGL(k_csr_raw, g2, bn, 0, st, N, E, ei, ew, w.ptr_dst, w.eid_dst, w.nbr_dst, w.wn_dst, w.ptr_src, w.eid_src, w.nbr_src,
                     w.wn_src, w.end_dst, w.end_src, w.deg);
}

dim3 panel_grid(int N, int hidden) { return dim3((unsigned)(((size_t)N * (hidden >> 2) + 255) / 256)); }
dim3 thin_grid(int N, int cols) { return dim3((cols + 255) / 256, (N + kThinRows - 1) / kThinRows); }

void acc(hipStream_t st, size_t n, float *a, const float *t, const float *u = nullptr) {
  hipLaunchKernelGGL(k_acc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, a, t, u);
}

bool ggnn_args_ok(int n_nodes, int n_edges, int in_dim, int hidden, int n_layers, int out_dim) {
  return n_nodes > 0 && n_edges >= 0 && in_dim > 0 && in_dim <= 8 && in_dim <= hidden && hidden > 0 && !(hidden & 3) && n_layers >= 1 &&
         n_layers <= kGgnnMaxLayers && out_dim > 0;
}

}  // namespace

extern "C" {

size_t drlgx_ggnn_workspace_bytes(int n_nodes, int n_edges, int hidden, int n_layers, int out_dim) {
  if (n_nodes <= 0 || n_edges < 0 || hidden <= 0 || n_layers < 1 || n_layers > kGgnnMaxLayers || out_dim <= 0) return 0;
  GgnnWs sizing;
  return carve(sizing, nullptr, n_nodes, std::max(n_edges, 1), hidden, n_layers) + 256;
}

int drlgx_ggnn_forward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int n_layers, int out_dim, const float *x,
                       const int64_t *edge_index, const float *edge_attr, const float *weight, const float *w_ih, const float *w_hh,
                       const float *b_ih, const float *b_hh, const float *Wf, const float *bf, const float *dropout_mask, float *out,
                       void *ws_dev, int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_edges_per_graph) {
  if (!ggnn_args_ok(n_nodes, n_edges, in_dim, hidden, n_layers, out_dim) || !x || !weight || !w_ih || !w_hh || !b_ih || !b_hh || !Wf || !bf ||
      !out || !ws_dev || (n_edges > 0 && (!edge_index || !edge_attr)) || (n_graphs > 0 && (!node_off || !edge_off || max_edges_per_graph < 0)))
    return DRLGX_E_INVALID;
  // (the gate and layer-0 kernels read the biases, the mask and weight[0] by 16-byte loads)
  if ((reinterpret_cast<uintptr_t>(b_ih) | reinterpret_cast<uintptr_t>(b_hh) | reinterpret_cast<uintptr_t>(dropout_mask) | reinterpret_cast<uintptr_t>(weight)) & 15)
    return DRLGX_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int N = n_nodes, C = hidden, C3 = 3 * hidden;
  GgnnWs w;
  carve(w, reinterpret_cast<char *>(ws_dev), N, std::max(n_edges, 1), C, n_layers);
  if (n_graphs > 0 && max_edges_per_graph <= kRawMaxEdges) {
    hipLaunchKernelGGL(k_csr_graphs_raw, dim3(n_graphs), dim3(256), 0, st, n_edges, edge_index, edge_attr, node_off, edge_off, w.deg, w.selfw,
                       w.ptr_dst, w.end_dst, w.nbr_dst, w.wn_dst, w.ptr_src, w.end_src, w.nbr_src, w.wn_src);
  } else {
    build_graph_raw(st, w, N, n_edges, edge_index, edge_attr);
  }
  const dim3 gp = panel_grid(N, C), b256(256);
  for (int l = 0; l < n_layers; ++l) {
    const GgnnLayer &y = w.layer[l];
    const bool last = l == n_layers - 1;
    const float *Wl = weight + (size_t)l * C * C;
    float *hout = last ? w.Hm : w.layer[l + 1].H;
    if (l == 0) {
      hipLaunchKernelGGL(k_ax, dim3((N * 8 + 255) / 256), b256, 0, st, N, in_dim, x, w.deg, w.selfw, w.ptr_dst, w.end_dst, w.nbr_dst, w.wn_dst, y.AH);
      hipLaunchKernelGGL(k_thin_nn, thin_grid(N, C >> 2), b256, 0, st, N, in_dim, C, y.AH, Wl, y.A);
      hipLaunchKernelGGL(k_thin_nt, thin_grid(N, C3), b256, 0, st, N, in_dim, C3, x, w_hh, C, w.GH);
    } else {
      hipLaunchKernelGGL(k_aggregate<false>, dim3(N), b256, 0, st, N, C, y.H, w.deg, w.selfw, w.ptr_dst, w.end_dst, w.nbr_dst, w.wn_dst, 0,
                         nullptr, nullptr, nullptr, y.AH);
      gemm<false, false, 0>(st, N, C, C, y.AH, C, Wl, C, y.A, C, nullptr, nullptr, 1);       // a = (A h) W_l
      gemm<false, true, 0>(st, N, C3, C, y.H, C, w_hh, C, w.GH, C3, nullptr, nullptr, 1);    // gh = h W_hh^T
    }
    gemm<false, true, 0>(st, N, C3, C, y.A, C, w_ih, C, w.GI, C3, nullptr, nullptr, 1);      // gi = a W_ih^T
#define DRLGX_GATE(THIN, LAST)                                                                                                           \
  hipLaunchKernelGGL((k_gru_gate<THIN, LAST>), gp, b256, 0, st, N, C, in_dim, w.GI, w.GH, THIN ? x : y.H, b_ih, b_hh, dropout_mask, hout, \
                     y.R, y.Z, y.Nn, y.HN)
    if (l == 0 && last) DRLGX_GATE(true, true);
    else if (l == 0) DRLGX_GATE(true, false);
    else if (last) DRLGX_GATE(false, true);
    else DRLGX_GATE(false, false);
#undef DRLGX_GATE
  }
  if (out_dim <= kThinOut)  // one pass over Hm (HBM-bound)
    hipLaunchKernelGGL(k_linear_out, dim3((N + 3) / 4), b256, 0, st, N, C, out_dim, w.Hm, Wf, bf, out);
  else  // the critic's 100 outputs: a product for the matrix cores
    gemm<false, true, 2>(st, N, out_dim, C, w.Hm, C, Wf, C, out, out_dim, bf, nullptr, 1);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_ggnn_backward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int n_layers, int out_dim, const float *x,
                        const int64_t *edge_index, const float *edge_attr, const float *weight, const float *w_ih, const float *w_hh,
                        const float *Wf, const float *dropout_mask, const float *d_out, float *d_weight, float *d_w_ih, float *d_w_hh,
                        float *d_b_ih, float *d_b_hh, float *dWf, float *dbf, void *ws_dev) {
  if (!ggnn_args_ok(n_nodes, n_edges, in_dim, hidden, n_layers, out_dim) || !x || !weight || !w_ih || !w_hh || !Wf || !d_out || !d_weight ||
      !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh || !dWf || !dbf || !ws_dev)
    return DRLGX_E_INVALID;
  (void)edge_index; (void)edge_attr;  // the forward left both CSRs and every layer's h, A h, a, r, z, n, hn in ws
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int N = n_nodes, C = hidden, C3 = 3 * hidden;
  const size_t CC = (size_t)C * C;
  GgnnWs w;
  carve(w, reinterpret_cast<char *>(ws_dev), N, std::max(n_edges, 1), C, n_layers);
  const dim3 gp = panel_grid(N, C), b256(256);
  // the GRU's gradients are sums over the layers; dweight[0] has in_dim live rows
  hipMemsetAsync(d_w_ih, 0, 3 * CC * sizeof(float), st);
  hipMemsetAsync(d_w_hh, 0, 3 * CC * sizeof(float), st);
  hipMemsetAsync(d_b_ih, 0, (size_t)C3 * sizeof(float), st);
  hipMemsetAsync(d_b_hh, 0, (size_t)C3 * sizeof(float), st);
  hipMemsetAsync(d_weight, 0, CC * sizeof(float), st);
  // read-out layer: D0 = dh_L = (dOut Wf) * (Hm > 0) * mask, as the GCN's dZ2 (Hm plays H2)
  float *dh = w.D0, *dh_next = w.D1;
  const uintptr_t al16 = reinterpret_cast<uintptr_t>(Wf) | reinterpret_cast<uintptr_t>(dropout_mask);
  if (out_dim <= kThinOut && (al16 & 15) == 0) {
    int rpb;
    const int nb = thin_slices(N, (size_t)out_dim + 1, C, w.part_floats, rpb);
    hipLaunchKernelGGL(k_dz2_sums, dim3((C / 4 + 63) / 64, nb), b256, 0, st, N, C, out_dim, d_out, Wf, dropout_mask, w.Hm, dh, w.part, rpb);
    hipLaunchKernelGGL(k_thin_tn_reduce, dim3(((out_dim + 1) * C + 63) / 64 + 1), dim3(1024), 0, st, C, out_dim, nb, w.part, dWf, out_dim,
                       (float *)nullptr, d_out, out_dim, N, dbf);
  } else if (out_dim <= kThinOut) {
    thin_tn(st, w.part, w.part_floats, out_dim, C, N, d_out, out_dim, w.Hm, C, dWf, out_dim, nullptr, dbf);
    hipLaunchKernelGGL(k_dz2, dim3(N), b256, 0, st, N, C, out_dim, d_out, Wf, dropout_mask, w.Hm, dh);
  } else {
    gemm_tn_splitk(st, w.part, w.part_floats, out_dim, C, N, d_out, out_dim, w.Hm, C, dWf, 32);
    colsum(st, w.part, w.part_floats, N, out_dim, d_out, dbf);
    gemm<false, false, 3>(st, N, C, out_dim, d_out, out_dim, Wf, C, dh, C, w.Hm, dropout_mask, 1);
  }
  for (int l = n_layers - 1; l >= 0; --l) {
    const GgnnLayer &y = w.layer[l];
    const float *Wl = weight + (size_t)l * CC;
    float *dGI = w.GI, *dGH = w.GH;
    if (l == 0)
      hipLaunchKernelGGL(k_gru_gate_bwd<true>, gp, b256, 0, st, N, C, in_dim, dh, x, y.R, y.Z, y.Nn, y.HN, dGI, dGH, (float *)nullptr);
    else
      hipLaunchKernelGGL(k_gru_gate_bwd<false>, gp, b256, 0, st, N, C, in_dim, dh, y.H, y.R, y.Z, y.Nn, y.HN, dGI, dGH, dh_next);
    // dW_ih += d(gi)^T a, per gate; db_ih += colsum(d(gi))
    for (int g = 0; g < 3; ++g) {
      gemm_tn_splitk(st, w.part, w.part_floats, C, C, N, dGI + (size_t)g * C, C3, y.A, C, w.TW);
      acc(st, CC, d_w_ih + g * CC, w.TW);
    }
    colsum(st, w.part, w.part_floats, N, C3, dGI, w.TB);
    acc(st, C3, d_b_ih, w.TB);
    // da = d(gi) W_ih
    gemm<false, false, 0>(st, N, C, C3, dGI, C3, w_ih, C, w.DA, C, nullptr, nullptr, 1);
    if (l == 0) {
      // h_0 = [x | 0]: dW_hh[:, :in_dim] += d(gh)^T x, db_hh += colsum(d(gh)) - one pass over d(gh); dweight[0][:in_dim] = AX^T da
      thin_tn(st, w.part, w.part_floats, in_dim, C3, N, x, in_dim, dGH, C3, w.TW, in_dim, w.TB);
      hipLaunchKernelGGL(k_acc_t, dim3((C3 + 255) / 256), b256, 0, st, C3, in_dim, C, d_w_hh, w.TW);
      acc(st, C3, d_b_hh, w.TB);
      thin_tn(st, w.part, w.part_floats, 8, C, N, y.AH, 8, w.DA, C, d_weight, in_dim, nullptr);
      break;
    }
    for (int g = 0; g < 3; ++g) {
      gemm_tn_splitk(st, w.part, w.part_floats, C, C, N, dGH + (size_t)g * C, C3, y.H, C, w.TW);
      acc(st, CC, d_w_hh + g * CC, w.TW);
    }
    colsum(st, w.part, w.part_floats, N, C3, dGH, w.TB);
    acc(st, C3, d_b_hh, w.TB);
    gemm_tn_splitk(st, w.part, w.part_floats, C, C, N, y.AH, C, w.DA, C, d_weight + (size_t)l * CC);  // dweight[l] = (A h)^T da
    gemm<false, false, 0>(st, N, C, C3, dGH, C3, w_hh, C, w.T1, C, nullptr, nullptr, 1);              // T1 = d(gh) W_hh
    gemm<false, true, 0>(st, N, C, C, w.DA, C, Wl, C, w.T2, C, nullptr, nullptr, 1);                  // T2 = d(A h) = da W_l^T
    hipLaunchKernelGGL(k_aggregate<false>, dim3(N), b256, 0, st, N, C, w.T2, w.deg, w.selfw, w.ptr_src, w.end_src, w.nbr_src, w.wn_src, 0,
                       nullptr, nullptr, nullptr, w.T3);                                               // T3 = A^T d(A h)
    acc(st, (size_t)N * C, dh_next, w.T1, w.T3);  // dh_l = z dh' + T1 + T3
    std::swap(dh, dh_next);
  }
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

}  // extern "C"
