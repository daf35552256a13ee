// Graph normalisation and the two CSRs of the GCN (by destination for the forward aggregation, by source for the transposed one),
// rows in edge order: the generic count / scan / fill / sort / finish kernels (launched by build_graph, k_gcn.hip), the one-launch
// build of a batch of small graphs k_csr_graphs with its launcher, and the collation of per-graph cached rows k_csr_collate.
#pragma once
#include "drlgx_dev.h"

namespace {

// in/out degree counts for the two CSRs (the weighted degree is summed later in edge order: float atomics here would
// make deg - and through the ReLU gates the whole forward/backward - depend on the arrival order)
// An explicit self loop keeps its weight as the node's self term (PyG add_remaining_self_loops: only the REMAINING self
// loops get the fill value 2): selfw[n] is preset to 2 and overwritten here.  Edges with an endpoint outside [0, N) are
// ignored (the C ABI has no status word for the GCN calls).
__global__ void k_degree(int N, int E, const int64_t *ei, const float *ew, int *cnt_dst, int *cnt_src, float *selfw) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t r64 = ei[e], c64 = ei[(size_t)E + e];
  if (r64 < 0 || r64 >= N || c64 < 0 || c64 >= N) return;
  const int r = (int)r64, c = (int)c64;
  if (r == c) {
    selfw[r] = ew[e];
    return;
  }
  atomicAdd(&cnt_dst[c], 1);
  atomicAdd(&cnt_src[r], 1);
}
// exclusive scan of two count arrays (single block of 1024 threads; N is a few 10^4): per-thread chunk sums, a
// shuffle scan inside each wave, a shuffle scan of the 16 wave totals, then the chunks are rewritten
__global__ __launch_bounds__(1024) void k_scan2(int n, const int *a, int *pa, const int *b, int *pb) {
  __shared__ int wtot[2][16];
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6;
  const int chunk = (n + nt - 1) / nt;
  const int i0 = t * chunk, i1 = min(n, i0 + chunk);
  int sa = 0, sb = 0;
  for (int i = i0; i < i1; ++i) {
    sa += a[i];
    sb += b[i];
  }
  int xa = sa, xb = sb;  // inclusive scan over the wave
  for (int off = 1; off < 64; off <<= 1) {
    const int ya = __shfl_up(xa, off), yb = __shfl_up(xb, off);
    if (lane >= off) {
      xa += ya;
      xb += yb;
    }
  }
  if (lane == 63) {
    wtot[0][wave] = xa;
    wtot[1][wave] = xb;
  }
  __syncthreads();
  if (wave == 0) {
    int va = lane < 16 ? wtot[0][lane] : 0, vb = lane < 16 ? wtot[1][lane] : 0;
    const int ia = va, ib = vb;
    for (int off = 1; off < 16; off <<= 1) {
      const int ya = __shfl_up(va, off), yb = __shfl_up(vb, off);
      if (lane >= off) {
        va += ya;
        vb += yb;
      }
    }
    if (lane < 16) {
      wtot[0][lane] = va - ia;  // exclusive
      wtot[1][lane] = vb - ib;
    }
    if (lane == 15) {
      pa[n] = va;
      pb[n] = vb;
    }
  }
  __syncthreads();
  sa = wtot[0][wave] + xa - sa;  // exclusive prefix of this thread's chunk
  sb = wtot[1][wave] + xb - sb;
  for (int i = i0; i < i1; ++i) {
    pa[i] = sa;
    sa += a[i];
    pb[i] = sb;
    sb += b[i];
  }
}
__global__ void k_csr_fill(int N, int E, const int64_t *ei, const int *ptr_dst, int *cur_dst, int *eid_dst, const int *ptr_src,
                           int *cur_src, int *eid_src) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t r64 = ei[e], c64 = ei[(size_t)E + e];
  if (r64 < 0 || r64 >= N || c64 < 0 || c64 >= N || r64 == c64) return;
  const int r = (int)r64, c = (int)c64;
  eid_dst[ptr_dst[c] + atomicAdd(&cur_dst[c], 1)] = e;
  eid_src[ptr_src[r] + atomicAdd(&cur_src[r], 1)] = e;
}
// sort each CSR row by edge id (rows are short) -> deterministic summation order; both CSRs in one launch
__global__ void k_csr_sort(int N, const int *ptr0, int *eid0, const int *ptr1, int *eid1) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= 2 * N) return;
  const int *ptr = n < N ? ptr0 : ptr1;
  int *eid = n < N ? eid0 : eid1;
  if (n >= N) n -= N;
  const int a = ptr[n], b = ptr[n + 1];
  for (int i = a + 1; i < b; ++i) {
    int v = eid[i], j = i - 1;
    while (j >= a && eid[j] > v) {
      eid[j + 1] = eid[j];
      --j;
    }
    eid[j + 1] = v;
  }
}
// deg[row] = sum of the row's edge weights in edge order, then the self loop weight (2 from
// add_remaining_self_loops(fill_value = 2), or the explicit self loop's own)  (PyG: scatter_add(edge_weight, row), row = source)
__global__ void k_degree_sum(int N, const float *ew, const int *ptr_src, const int *eid_src, const float *selfw, float *deg) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int i = ptr_src[n]; i < ptr_src[n + 1]; ++i) s += ew[eid_src[i]];
  deg[n] = s + selfw[n];
}
// resolve (neighbour, normalised weight) per CSR slot, for the by-destination CSR (threads < N) and the by-source one.
// dis = deg^-1/2 (inf -> 0).
__global__ void k_csr_finish(int N, int E, const int64_t *ei, const float *ew, const float *deg, const int *ptr_dst,
                             const int *eid_dst, int *nbr_dst, float *wn_dst, const int *ptr_src, const int *eid_src, int *nbr_src,
                             float *wn_src, int *end_dst, int *end_src) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= 2 * N) return;
  const bool by_dst = n < N;
  const int *ptr = by_dst ? ptr_dst : ptr_src, *eid = by_dst ? eid_dst : eid_src;
  int *nbr = by_dst ? nbr_dst : nbr_src;
  float *wn = by_dst ? wn_dst : wn_src;
  if (!by_dst) n -= N;
  (by_dst ? end_dst : end_src)[n] = ptr[n + 1];
  for (int i = ptr[n]; i < ptr[n + 1]; ++i) {
    const int e = eid[i];
    const int r = (int)ei[e], c = (int)ei[(size_t)E + e];
    float dr = deg[r] > 0 ? 1.0f / sqrtf(deg[r]) : 0.0f, dc = deg[c] > 0 ? 1.0f / sqrtf(deg[c]) : 0.0f;
    nbr[i] = by_dst ? r : c;
    wn[i] = dr * ew[e] * dc;  // deg^-1/2[row] * w * deg^-1/2[col]
  }
}

// ------------------------------------------------------------------------------------------------
// Both CSRs, the degrees and the normalised weights of a BATCH of small graphs in one launch: one workgroup per graph
// (a PyG batch / drlgx_graph export: graph g owns nodes [node_off[g], node_off[g+1]) and edges [edge_off[g],
// edge_off[g+1]), every edge connects two of its nodes).  The graph's edges are sorted in LDS by (source node, edge id)
// and by (destination node, edge id) - one 32-bit key each, two bitonic sorts run stage by stage together -, which IS
// the CSR order of the generic build (rows by node, entries in edge order): the same rows, bit for bit, without its
// eight launches (k_degree .. k_csr_finish are dominated by launch latency at these sizes).
// Row r of graph g starts at edge_off[g] + (position of its first key): rows are contiguous inside a graph; self loops
// and ignored edges sort to the end and leave unused slots there, hence explicit row ends.
// ------------------------------------------------------------------------------------------------
constexpr int kCsrKeyShift = 14;               // key = local node << 14 | local edge id
constexpr int kCsrMaxEdges = 1 << kCsrKeyShift;  // per graph (16 384; 2 x 64 KB of keys in LDS at that size)
constexpr uint32_t kCsrNoKey = 0xffffffffu;

__global__ __launch_bounds__(256) void k_csr_graphs(int N, int E, int P2, int extra, const int64_t *ei, const float *ew, const int *node_off,
                                                    const int *edge_off, float *deg, float *selfw_out, int *ptr_dst, int *end_dst,
                                                    int *nbr_dst, float *wn_dst, int *ptr_src, int *end_src, int *nbr_src, float *wn_src,
                                                    const float *x, int in_dim, float *AX, int local) {
  // local (the replay pool's per-graph cache, drlgx_replay_cache_csr): row starts / ends and neighbour ids are stored relative
  // to the graph's first edge / node, so that a later collation only adds the graph's offsets in the mini-batch
  extern __shared__ uint32_t s_keys[];  // [2][P2]: by source, by destination; then (extra) the weights and packed endpoints
  uint32_t *ks = s_keys, *kd = s_keys + P2;
  float *s_w = reinterpret_cast<float *>(s_keys + 2 * (size_t)P2);
  uint32_t *s_pk = s_keys + 3 * (size_t)P2;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n0 = node_off[g], n1 = node_off[g + 1], e0 = edge_off[g];
  const int ng = n1 - n0, eg = min(edge_off[g + 1] - e0, P2);  // (the caller promised eg <= P2)
  const int eb = local ? 0 : e0, nb = local ? 0 : n0;  // what stored positions / ids are relative to
  const bool ext = extra && ng <= 65535;  // the edges' weights and local endpoints stay in LDS: the later passes read no edge from memory
  for (int m = tid; m < ng; m += 256) selfw_out[n0 + m] = 2.0f;  // add_remaining_self_loops(fill_value = 2)
  __syncthreads();
  for (int j = tid; j < P2; j += 256) {
    uint32_t a = kCsrNoKey, b = kCsrNoKey;
    if (j < eg) {
      const int64_t r = ei[e0 + j], c = ei[(size_t)E + e0 + j];
      const float wj = ew[e0 + j];
      if (ext) s_w[j] = wj;
      if (r >= n0 && r < n1 && c >= n0 && c < n1) {  // an edge with an endpoint outside the graph is ignored
        if (ext) s_pk[j] = (uint32_t)(r - n0) | ((uint32_t)(c - n0) << 16);
        if (r == c) {
          selfw_out[r] = wj;  // an explicit self loop keeps its weight as the node's self term
        } else {
          a = ((uint32_t)(r - n0) << kCsrKeyShift) | (uint32_t)j;
          b = ((uint32_t)(c - n0) << kCsrKeyShift) | (uint32_t)j;
        }
      }
    }
    ks[j] = a;
    kd[j] = b;
  }
  __syncthreads();
  // bitonic sort, ascending, both key arrays in the same stages.  Wave w owns the contiguous segment of P2 / 4 keys
  // [w P2/4, (w+1) P2/4): a compare-exchange at distance j < P2/4 stays inside the segment, and a wave's LDS operations
  // execute in order, so only the stages that cross segments (three of the 55 at P2 = 1024) take workgroup barriers
  {
    const int seg = P2 >> 2, wave = tid >> 6, lane = tid & 63;
    auto exchange = [&](int t, int k, int j) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
      const bool up = (i & k) == 0;
      const uint32_t a0 = ks[i], a1 = ks[q], b0 = kd[i], b1 = kd[q];
      const uint32_t alo = min(a0, a1), ahi = max(a0, a1), blo = min(b0, b1), bhi = max(b0, b1);
      ks[i] = up ? alo : ahi;  // (unconditional stores: no divergent branches in the 55 stages)
      ks[q] = up ? ahi : alo;
      kd[i] = up ? blo : bhi;
      kd[q] = up ? bhi : blo;
    };
    for (int k = 2; k <= P2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        if (seg >= 64 && j < seg) {  // inside the segments: this wave's seg / 2 pairs, wave-level ordering only
          for (int u = lane; u < (seg >> 1); u += 64) exchange(wave * (seg >> 1) + u, k, j);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {                      // across segments (or a tiny sort): other waves' results in, other waves' operands out
          __syncthreads();
          for (int t = tid; t < (P2 >> 1); t += 256) exchange(t, k, j);
          __syncthreads();
        }
      }
    __syncthreads();
  }
  // rows = key ranges; weighted degree = the by-source row summed in edge order, then the self term
  auto lower = [&](const uint32_t *keys, uint32_t v) {
    int lo = 0, hi = P2;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  for (int m = tid; m < ng; m += 256) {
    const uint32_t v0 = (uint32_t)m << kCsrKeyShift, v1 = (uint32_t)(m + 1) << kCsrKeyShift;
    const int s0 = lower(ks, v0), s1 = lower(ks, v1), d0 = lower(kd, v0), d1 = lower(kd, v1);
    const int n = n0 + m;
    ptr_src[n] = eb + s0;
    end_src[n] = eb + s1;
    ptr_dst[n] = eb + d0;
    end_dst[n] = eb + d1;
    float dsum = 0.f;
    for (int i = s0; i < s1; ++i) {
      const int j = (int)(ks[i] & (kCsrMaxEdges - 1));
      dsum += ext ? s_w[j] : ew[e0 + j];
    }
    deg[n] = dsum + selfw_out[n];
  }
  __threadfence_block();  // deg[] of the whole graph is read below
  __syncthreads();
  // entries: (neighbour, deg^-1/2[row] w deg^-1/2[col]), one thread per sorted position
  for (int i = tid; i < eg; i += 256) {
    const uint32_t a = ks[i], b = kd[i];
    if (a != kCsrNoKey) {
      const int j = (int)(a & (kCsrMaxEdges - 1));
      const int r = n0 + (int)(a >> kCsrKeyShift), c = ext ? n0 + (int)(s_pk[j] >> 16) : (int)ei[(size_t)E + e0 + j];
      const float dr = deg[r] > 0 ? 1.0f / sqrtf(deg[r]) : 0.0f, dc = deg[c] > 0 ? 1.0f / sqrtf(deg[c]) : 0.0f;
      nbr_src[e0 + i] = c - n0 + nb;
      wn_src[e0 + i] = dr * (ext ? s_w[j] : ew[e0 + j]) * dc;
    }
    if (b != kCsrNoKey) {
      const int j = (int)(b & (kCsrMaxEdges - 1));
      const int c = n0 + (int)(b >> kCsrKeyShift), r = ext ? n0 + (int)(s_pk[j] & 0xffffu) : (int)ei[e0 + j];
      const float dr = deg[r] > 0 ? 1.0f / sqrtf(deg[r]) : 0.0f, dc = deg[c] > 0 ? 1.0f / sqrtf(deg[c]) : 0.0f;
      nbr_dst[e0 + i] = r - n0 + nb;
      wn_dst[e0 + i] = dr * (ext ? s_w[j] : ew[e0 + j]) * dc;
    }
  }
  if (!AX) return;
  // AX = Â X of the graph's own nodes (k_ax's expression and order), from the rows this workgroup has just written
  __threadfence_block();
  __syncthreads();
  for (int e = tid; e < ng * 8; e += 256) {
    const int n = n0 + (e >> 3), t = e & 7;
    float s = 0.f;
    if (t < in_dim) {
      s = (selfw_out[n] / deg[n]) * x[(size_t)n * in_dim + t];
      for (int i = ptr_dst[n] + (e0 - eb); i < end_dst[n] + (e0 - eb); ++i) s += wn_dst[i] * x[(size_t)(nbr_dst[i] + (n0 - nb)) * in_dim + t];
    }
    AX[(size_t)n * 8 + t] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// Mini-batch collation of replay graphs whose normalisation, CSRs and ÂX were cached per graph when their export entered the
// pool (k_csr_graphs in `local` mode): graph g of the mini-batch (desc int64 [5][G] = node_start, node_cnt, edge_start,
// edge_cnt, loc, as k_replay_collate) is copied into the GCN workspace's arrays at its cumulative node / edge offsets, row
// starts / ends shifted by the edge offset, neighbour ids by the node offset - what build_graph_batched + the ÂX pass would
// have produced for the collated batch, bit for bit (the per-graph sort order does not depend on where the graph sits).
// Blocks [G, 2G): the second list's cached per-node value only (the target read-out over the next states), as
// k_replay_collate's pair form.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_csr_collate(int G, const int64_t *desc, drlgx_csr_cache c, float *deg, float *selfw, float *AX,
                                                     int *ptr_dst, int *end_dst, int *ptr_src, int *end_src, int *nbr_dst, int *nbr_src,
                                                     float *wn_dst, float *wn_src, int *node_off_out, int *edge_off_out,
                                                     const int64_t *desc2, const float *pool_q, float *q2_out) {
  __shared__ long long red[2][4];
  const int tid = threadIdx.x;
  int g = blockIdx.x;
  const bool second = g >= G;
  if (second) {
    g -= G;
    desc = desc2;
  }
  long long sn = 0, se = 0;
  for (int j = tid; j < g; j += 256) {
    sn += desc[(size_t)G + j];
    se += desc[3 * (size_t)G + j];
  }
  for (int o = 32; o > 0; o >>= 1) {
    sn += __shfl_down(sn, o);
    se += __shfl_down(se, o);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sn;
    red[1][tid >> 6] = se;
  }
  __syncthreads();
  const long long node_off = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const long long edge_off = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  const long long n0 = desc[g], nn = desc[(size_t)G + g], e0 = desc[2 * (size_t)G + g], ne = desc[3 * (size_t)G + g];
  if (second) {
    for (long long i = tid; i < nn; i += 256) q2_out[node_off + i] = pool_q[n0 + i];
    return;
  }
  if (tid == 0) {
    node_off_out[g] = (int)node_off;
    edge_off_out[g] = (int)edge_off;
    if (g == G - 1) {
      node_off_out[G] = (int)(node_off + nn);
      edge_off_out[G] = (int)(edge_off + ne);
    }
  }
  const int eo = (int)edge_off, no = (int)node_off;
  for (long long i = tid; i < nn; i += 256) {
    deg[node_off + i] = c.deg[n0 + i];
    selfw[node_off + i] = c.selfw[n0 + i];
    ptr_dst[node_off + i] = c.ptr_dst[n0 + i] + eo;
    end_dst[node_off + i] = c.end_dst[n0 + i] + eo;
    ptr_src[node_off + i] = c.ptr_src[n0 + i] + eo;
    end_src[node_off + i] = c.end_src[n0 + i] + eo;
  }
  {
    const float4 *s4 = reinterpret_cast<const float4 *>(c.ax + n0 * 8);
    float4 *d4 = reinterpret_cast<float4 *>(AX + node_off * 8);
    for (long long i = tid; i < nn * 2; i += 256) d4[i] = s4[i];
  }
  for (long long j = tid; j < ne; j += 256) {
    nbr_dst[edge_off + j] = c.nbr_dst[e0 + j] + no;
    nbr_src[edge_off + j] = c.nbr_src[e0 + j] + no;
    wn_dst[edge_off + j] = c.wn_dst[e0 + j];
    wn_src[edge_off + j] = c.wn_src[e0 + j];
  }
}
// The one launch of k_csr_graphs: `out` (a drlgx_csr_cache: the replay pool's, or the same arrays of a GCN workspace) receives
// the rows of n_graphs graphs, out.ax = Â X beside them.  ei_stride: the kernel reads the second row of edge_index at ei[ei_stride + e].
// false: a graph may have more edges than the kernel sorts in LDS (nothing launched).
bool launch_csr_graphs(hipStream_t st, int n_graphs, const int *node_off, const int *edge_off, int max_edges_per_graph, int N, int ei_stride,
                       const int64_t *ei, const float *ew, const float *x, int in_dim, const drlgx_csr_cache &out, int local) {
  if (max_edges_per_graph > kCsrMaxEdges) return false;
  int P2 = 64;
  while (P2 < max_edges_per_graph) P2 <<= 1;
  const int extra = P2 <= 4096 ? 1 : 0;  // weights + packed endpoints beside the keys: 16 bytes per edge slot, <= 64 KB
  const size_t lds = (size_t)(extra ? 4 : 2) * P2 * sizeof(uint32_t);
  static bool attr_set[32] = {false};
  const void *fns[] = {reinterpret_cast<const void *>(&k_csr_graphs)};
  drlgx_ensure_lds_attr(attr_set, fns, 1, 160 * 1024);
  hipLaunchKernelGGL(k_csr_graphs, dim3(n_graphs), dim3(256), lds, st, N, ei_stride, P2, extra, ei, ew, node_off, edge_off, out.deg, out.selfw,
                     out.ptr_dst, out.end_dst, out.nbr_dst, out.wn_dst, out.ptr_src, out.end_src, out.nbr_src, out.wn_src, x, in_dim, out.ax, local);
  return true;
}

}  // namespace
