// GCN policy network on gfx950: forward and backward of
//   H1 = relu(Â X W1 + b1),  H2 = relu(Â H1 W2 + b2) [* dropout mask],  out = H2 Wf^T + bf
// with Â = D^-1/2 (A_w + 2I) D^-1/2, D = rowsum(A_w + 2I)   (PyG 1.x GCNConv(improved=True), SURVEY.md App. B;
// scripts/Networks.py:12-70 GCN / PolicyGCN / ValueGCN trunks; scripts/policy.py:234-253 for the backward).
//
// Layout / kernels (k_gcn_csr.hip, k_gcn_agg.hip, k_gemm.hip, k_gcn_thin.hip; this file: the workspace and the C entry points)
//   * the batch is irregular (one graph per env): edges are turned into two CSRs (by destination for the
//     forward aggregation, by source for the transposed one) with deterministic per-row order - per graph in ONE launch
//     when the caller knows the batch's graph boundaries (k_csr_graphs: the graph's edges sorted in LDS), else by the
//     generic count / scan / fill / sort / finish sequence;
//   * layer 1 (K = 5) is never materialised: AX = Â X is 8 floats per node (k_ax), and the aggregation of layer 2
//     recomputes the rows of H1 = relu(AX W1 + b1) it gathers (k_aggregate_l1; the backward pass recomputes the ReLU gate);
//   * aggregation (Â H): float4 lanes across the 1000 features, neighbour rows gathered with coalesced 4 KB reads;
//   * the dense 1000x1000 contractions run on the fp32 matrix cores (exact fp32, 157 TFLOP/s peak) with a fused
//     bias+ReLU(+mask) epilogue: batches large enough to fill the chip with (96..160) x 128 tiles on k_gemm_wide (8 waves,
//     v_mfma_f32_16x16x4_f32, tile height picked per launch), smaller ones on the 64x64 kernels (4 waves of one 32x32 MFMA
//     tile); operand tiles global -> LDS directly in both; the weight-gradient products (K = #nodes) use split-K with a
//     deterministic second-stage reduction.
// fp32 throughout (the reference trains in fp32); (Â X) W1 is used instead of Â (X W1) — same value up to fp32
// rounding (tests: <= 2e-5 relative against the plain-torch reference).
#include <algorithm>

#include "k_gemm.hip"
#include "k_gcn_csr.hip"
#include "k_gcn_agg.hip"
#include "k_gcn_thin.hip"

namespace {

struct GcnWs {
  float *deg, *selfw, *wn_dst, *wn_src, *AX, *b1s, *AH1, *H2, *T0, *T1, *part;
  int *cnt_dst, *cnt_src, *ptr_dst, *ptr_src, *cur_dst, *cur_src, *eid_dst, *eid_src, *nbr_dst, *nbr_src, *end_dst, *end_src;
  size_t part_floats, counters_bytes;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// lays the workspace out from `base` (null: for its size only, the pointers are then offsets) and returns its bytes
size_t carve(GcnWs &w, char *base, int N, int E, int hidden) {
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
  const size_t part = std::max<size_t>((size_t)8 * hidden * hidden, (size_t)64 * hidden);
  takef(w.deg, N);
  takef(w.selfw, N);
  takef(w.wn_dst, E);
  takef(w.wn_src, E);
  takef(w.AX, (size_t)N * 8);
  takef(w.b1s, hidden);  // the forward's b1, for the backward's layer-1 ReLU gate (H1 is recomputed, not stored)
  takef(w.AH1, NH);
  takef(w.H2, NH);
  takef(w.T0, NH);
  takef(w.T1, NH);
  takef(w.part, part);
  w.part_floats = part;
  takei(w.cnt_dst, N + 1);  // the four counters are contiguous: one memset (see build_graph)
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

// normalisation and both CSRs of any edge list into the workspace: the generic sequence of k_gcn_csr.hip
void build_graph(hipStream_t st, const GcnWs &w, int N, int E, const int64_t *ei, const float *ew) {
  hipMemsetAsync(w.cnt_dst, 0, w.counters_bytes, st);  // cnt_dst, cnt_src, cur_dst, cur_src
  hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.selfw), 0x40000000, (size_t)N, st);  // 2.0f: the improved-GCN fill value
  if (E > 0) hipLaunchKernelGGL(k_degree, dim3((E + 255) / 256), dim3(256), 0, st, N, E, ei, ew, w.cnt_dst, w.cnt_src, w.selfw);
  hipLaunchKernelGGL(k_scan2, dim3(1), dim3(1024), 0, st, N, w.cnt_dst, w.ptr_dst, w.cnt_src, w.ptr_src);
  if (E > 0) {
    hipLaunchKernelGGL(k_csr_fill, dim3((E + 255) / 256), dim3(256), 0, st, N, E, ei, w.ptr_dst, w.cur_dst, w.eid_dst, w.ptr_src,
                       w.cur_src, w.eid_src);
  }
  const dim3 gn((N + 127) / 128), g2((2 * N + 127) / 128), bn(128);
  hipLaunchKernelGGL(k_csr_sort, g2, bn, 0, st, N, w.ptr_dst, w.eid_dst, w.ptr_src, w.eid_src);
  hipLaunchKernelGGL(k_degree_sum, gn, bn, 0, st, N, ew, w.ptr_src, w.eid_src, w.selfw, w.deg);
  hipLaunchKernelGGL(k_csr_finish, g2, bn, 0, st, N, E, ei, ew, w.deg, w.ptr_dst, w.eid_dst, w.nbr_dst, w.wn_dst, w.ptr_src,
                     w.eid_src, w.nbr_src, w.wn_src, w.end_dst, w.end_src);
}

// the same in one launch when the caller knows the batch's graph boundaries; AX = Â X comes out of it too (k_ax otherwise).
// false: a graph has more edges than k_csr_graphs sorts (the caller falls back to build_graph)
bool build_graph_batched(hipStream_t st, const GcnWs &w, int N, int E, const int64_t *ei, const float *ew, int G, const int *node_off,
                         const int *edge_off, int max_edges_per_graph, const float *x, int in_dim) {
  const drlgx_csr_cache rows = {w.deg, w.selfw, w.AX, w.ptr_dst, w.end_dst, w.ptr_src, w.end_src, w.nbr_dst, w.nbr_src, w.wn_dst, w.wn_src};
  return launch_csr_graphs(st, G, node_off, edge_off, max_edges_per_graph, N, E, ei, ew, x, in_dim, rows, 0);
}

}  // namespace

extern "C" {

int drlgx_debug_gemm_tile_rows(int m, int n, int k_slices, int transpose_a) {
  const WidePick p = wide_pick(m, n, k_slices, transpose_a != 0);
  return p.rt ? 1000 * (16 * p.nw) + 16 * p.rt : 64064;
}

size_t drlgx_gcn_workspace_bytes(int n_nodes, int n_edges, int hidden, int out_dim) {
  if (n_nodes <= 0 || n_edges < 0 || hidden <= 0 || out_dim <= 0) return 0;
  GcnWs sizing;
  return carve(sizing, nullptr, n_nodes, std::max(n_edges, 1), hidden) + 256;
}

constexpr int kPrebuilt = -7;  // gcn_forward_impl's n_graphs: the graph part of the workspace is already built
static int gcn_forward_impl(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim, const float *x,
                            const int64_t *edge_index, const float *edge_attr, const float *W1, const float *b1, const float *W2,
                            const float *b2, const float *Wf, const float *bf, const float *dropout_mask, float *out, void *ws_dev,
                            int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_edges_per_graph) {
  const bool prebuilt = n_graphs == kPrebuilt;
  if (n_nodes <= 0 || n_edges < 0 || in_dim <= 0 || in_dim > 8 || hidden <= 0 || (hidden & 3) || out_dim <= 0 || (!x && !prebuilt) || !W1 ||
      !b1 || !W2 || !b2 || !Wf || !bf || !out || !ws_dev || (n_edges > 0 && !prebuilt && (!edge_index || !edge_attr)))
    return DRLGX_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  GcnWs w;
  carve(w, reinterpret_cast<char *>(ws_dev), n_nodes, std::max(n_edges, 1), hidden);
  if (n_graphs == kPrebuilt) {
    // normalisation, both CSRs and AX already are in the workspace (drlgx_gcn_collate_csr)
  } else if (n_graphs <= 0 ||
      !build_graph_batched(st, w, n_nodes, n_edges, edge_index, edge_attr, n_graphs, node_off, edge_off, max_edges_per_graph, x, in_dim)) {
    build_graph(st, w, n_nodes, n_edges, edge_index, edge_attr);
    hipLaunchKernelGGL(k_ax, dim3((n_nodes * 8 + 255) / 256), dim3(256), 0, st, n_nodes, in_dim, x, w.deg, w.selfw, w.ptr_dst, w.end_dst,
                       w.nbr_dst, w.wn_dst, w.AX);
  }
  {
    const dim3 ga((n_nodes + kAggNodes - 1) / kAggNodes), ba(256);
    if (in_dim == 5)  // the reference's feature count: compiled straight-line
      hipLaunchKernelGGL(k_aggregate_l1<5>, ga, ba, 0, st, n_nodes, in_dim, hidden, w.AX, W1, b1, w.deg, w.selfw, w.ptr_dst, w.end_dst, w.nbr_dst,
                         w.wn_dst, w.AH1, w.b1s);
    else
      hipLaunchKernelGGL(k_aggregate_l1<0>, ga, ba, 0, st, n_nodes, in_dim, hidden, w.AX, W1, b1, w.deg, w.selfw, w.ptr_dst, w.end_dst, w.nbr_dst,
                         w.wn_dst, w.AH1, w.b1s);
  }
  // H2 = relu(AH1 W2 + b2) * mask   (fp32 MFMA, fused epilogue)
  gemm<false, false, 1>(st, n_nodes, hidden, hidden, w.AH1, hidden, W2, hidden, w.H2, hidden, b2, dropout_mask, 1);
  if (out_dim <= kThinOut)  // one pass over H2 (HBM-bound)
    hipLaunchKernelGGL(k_linear_out, dim3((n_nodes + 3) / 4), dim3(256), 0, st, n_nodes, hidden, out_dim, w.H2, Wf, bf, out);
  else  // the critic's 100 outputs: a product for the matrix cores (k_linear_out walked H2's row once per output: 0.85 ms at 12.8 k nodes)
    gemm<false, true, 2>(st, n_nodes, out_dim, hidden, w.H2, hidden, Wf, hidden, out, out_dim, bf, nullptr, 1);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_gcn_forward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim, const float *x,
                      const int64_t *edge_index, const float *edge_attr, const float *W1, const float *b1, const float *W2,
                      const float *b2, const float *Wf, const float *bf, const float *dropout_mask, float *out, void *ws_dev) {
  return gcn_forward_impl(hip_stream, n_nodes, n_edges, in_dim, hidden, out_dim, x, edge_index, edge_attr, W1, b1, W2, b2, Wf, bf,
                          dropout_mask, out, ws_dev, 0, nullptr, nullptr, 0);
}

int drlgx_gcn_forward_batched(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim, const float *x,
                              const int64_t *edge_index, const float *edge_attr, const float *W1, const float *b1, const float *W2,
                              const float *b2, const float *Wf, const float *bf, const float *dropout_mask, float *out, void *ws_dev,
                              int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_edges_per_graph) {
  if (n_graphs <= 0 || !node_off || !edge_off || max_edges_per_graph < 0) return DRLGX_E_INVALID;
  return gcn_forward_impl(hip_stream, n_nodes, n_edges, in_dim, hidden, out_dim, x, edge_index, edge_attr, W1, b1, W2, b2, Wf, bf,
                          dropout_mask, out, ws_dev, n_graphs, node_off, edge_off, max_edges_per_graph);
}

int drlgx_gcn_forward_prebuilt(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim, const float *W1, const float *b1,
                               const float *W2, const float *b2, const float *Wf, const float *bf, const float *dropout_mask, float *out,
                               void *ws_dev) {
  return gcn_forward_impl(hip_stream, n_nodes, n_edges, in_dim, hidden, out_dim, nullptr, nullptr, nullptr, W1, b1, W2, b2, Wf, bf, dropout_mask,
                          out, ws_dev, kPrebuilt, nullptr, nullptr, 0);
}

static bool cache_ok(const drlgx_csr_cache *c) {
  return c && c->deg && c->selfw && c->ax && c->ptr_dst && c->end_dst && c->ptr_src && c->end_src && c->nbr_dst && c->nbr_src && c->wn_dst &&
         c->wn_src;
}

int drlgx_replay_cache_csr(void *hip_stream, int n_graphs, const int32_t *node_off, const int32_t *edge_off, int max_edges_per_graph,
                           const float *x, int in_dim, const int64_t *edge_index, int64_t edge_row_stride, const float *edge_attr,
                           const drlgx_csr_cache *cache) {
  if (n_graphs <= 0 || !node_off || !edge_off || max_edges_per_graph < 0 || !x || in_dim <= 0 || in_dim > 8 || !edge_index || !edge_attr ||
      edge_row_stride <= 0 || edge_row_stride >= (1ll << 31) || !cache_ok(cache))
    return DRLGX_E_INVALID;
  if (!launch_csr_graphs(reinterpret_cast<hipStream_t>(hip_stream), n_graphs, node_off, edge_off, max_edges_per_graph, 0, (int)edge_row_stride,
                         edge_index, edge_attr, x, in_dim, *cache, 1))
    return DRLGX_E_CAPACITY;  // (the caller keeps such an export uncached)
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_gcn_collate_csr(void *hip_stream, int n_graphs, const int64_t *desc_dev, const drlgx_csr_cache *cache, int n_nodes, int n_edges, int hidden,
                          int out_dim, void *ws_dev, int32_t *node_off_out, int32_t *edge_off_out, const int64_t *desc2_dev, const float *pool_q,
                          float *q2_out) {
  if (n_graphs <= 0 || !desc_dev || !cache_ok(cache) || n_nodes <= 0 || n_edges < 0 || hidden <= 0 || out_dim <= 0 || !ws_dev || !node_off_out ||
      !edge_off_out || (desc2_dev && (!pool_q || !q2_out)))
    return DRLGX_E_INVALID;
  GcnWs w;
  carve(w, reinterpret_cast<char *>(ws_dev), n_nodes, std::max(n_edges, 1), hidden);
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL(k_csr_collate, dim3(desc2_dev ? 2 * n_graphs : n_graphs), dim3(256), 0, st, n_graphs, desc_dev, *cache, w.deg, w.selfw, w.AX,
                     w.ptr_dst, w.end_dst, w.ptr_src, w.end_src, w.nbr_dst, w.nbr_src, w.wn_dst, w.wn_src, node_off_out, edge_off_out, desc2_dev,
                     pool_q, q2_out);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

int drlgx_gcn_backward(void *hip_stream, int n_nodes, int n_edges, int in_dim, int hidden, int out_dim, const float *x,
                       const int64_t *edge_index, const float *edge_attr, const float *W1, const float *W2, const float *Wf,
                       const float *dropout_mask, const float *d_out, float *dW1, float *db1, float *dW2, float *db2, float *dWf,
                       float *dbf, void *ws_dev) {
  if (n_nodes <= 0 || in_dim <= 0 || in_dim > 8 || hidden <= 0 || (hidden & 3) || out_dim <= 0 || !d_out || !dW1 || !db1 || !dW2 ||
      !db2 || !dWf || !dbf || !ws_dev || !W1 || !W2 || !Wf)
    return DRLGX_E_INVALID;
  (void)x; (void)edge_index; (void)edge_attr; (void)n_edges;  // the forward left AX / b1 / AH1 / H2 and both CSRs in ws
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  GcnWs w;
  carve(w, reinterpret_cast<char *>(ws_dev), n_nodes, std::max(n_edges, 1), hidden);
  // output layer
  const uintptr_t al16 = reinterpret_cast<uintptr_t>(Wf) | reinterpret_cast<uintptr_t>(dropout_mask) | reinterpret_cast<uintptr_t>(w.H2) |
                         reinterpret_cast<uintptr_t>(w.T0);
  if (out_dim <= kThinOut && (al16 & 15) == 0) {
    // dWf = dOut^T H2m, dbf = colsum(dOut), T0 = dZ2, db2 = colsum(dZ2): one pass over H2 and one reduce
    int rpb;
    const int nb = thin_slices(n_nodes, (size_t)out_dim + 1, hidden, w.part_floats, rpb);
    hipLaunchKernelGGL(k_dz2_sums, dim3((hidden / 4 + 63) / 64, nb), dim3(256), 0, st, n_nodes, hidden, out_dim, d_out, Wf, dropout_mask, w.H2, w.T0,
                       w.part, rpb);
    hipLaunchKernelGGL(k_thin_tn_reduce, dim3(((out_dim + 1) * hidden + 63) / 64 + 1), dim3(1024), 0, st, hidden, out_dim, nb, w.part, dWf, out_dim,
                       db2, d_out, out_dim, n_nodes, dbf);
  } else {
    if (out_dim <= kThinOut) {
      thin_tn(st, w.part, w.part_floats, out_dim, hidden, n_nodes, d_out, out_dim, w.H2, hidden, dWf, out_dim, nullptr, dbf);  // dWf = dOut^T H2m, dbf = colsum(dOut)
    } else {
      gemm_tn_splitk(st, w.part, w.part_floats, out_dim, hidden, n_nodes, d_out, out_dim, w.H2, hidden, dWf, 32);
      colsum(st, w.part, w.part_floats, n_nodes, out_dim, d_out, dbf);
    }
    // T0 = dZ2 = (dOut Wf) * gate
    if (out_dim <= kThinOut)
      hipLaunchKernelGGL(k_dz2, dim3(n_nodes), dim3(256), 0, st, n_nodes, hidden, out_dim, d_out, Wf, dropout_mask, w.H2, w.T0);
    else
      gemm<false, false, 3>(st, n_nodes, hidden, out_dim, d_out, out_dim, Wf, hidden, w.T0, hidden, w.H2, dropout_mask, 1);
    colsum(st, w.part, w.part_floats, n_nodes, hidden, w.T0, db2);
  }
  // layer 2
  gemm_tn_splitk(st, w.part, w.part_floats, hidden, hidden, n_nodes, w.AH1, hidden, w.T0, hidden, dW2);  // dW2 = AH1^T dZ2
  gemm<false, true, 0>(st, n_nodes, hidden, hidden, w.T0, hidden, W2, hidden, w.T1, hidden, nullptr, nullptr, 1);  // T1 = dZ2 W2^T
  // dZ1 = (Â^T dAH1) * (H1 > 0)   -> T0
  hipLaunchKernelGGL(k_aggregate<true>, dim3(n_nodes), dim3(256), 0, st, n_nodes, hidden, w.T1, w.deg, w.selfw, w.ptr_src, w.end_src, w.nbr_src,
                     w.wn_src, in_dim, w.AX, W1, w.b1s, w.T0);
  // layer 1
  thin_tn(st, w.part, w.part_floats, 8, hidden, n_nodes, w.AX, 8, w.T0, hidden, dW1, in_dim, db1);  // dW1 = AX^T dZ1 (AX rows are 8 wide), db1 = colsum(dZ1)
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}

}  // extern "C"
