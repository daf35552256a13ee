// Small kernels around the belief step: instance copies for the look-ahead (deep copies of
// SLAM2D / Simulator2D state, Planner2D.cpp:1417-1420), SLAM2D::set_copy_isam re-basing
// (SLAM2D.cpp:490-497), rewards / utility (Planner2D.cpp:354-366, 1463-1464) and the closed-form
// line planner (Planner2D.cpp:937-1041).
#include "drlgx_dev.h"
#include "drlgx_fields.h"

namespace {

// the incremental update's covariance panel (csrc/k_inc.hip) of instance s -> d: the live rows / columns only.  Block
// `part` of kCopySplit copies every kCopySplit-th group of 8 rows, 32 threads x 16 bytes per row, four rows' loads in
// flight per thread.  (Eight parts since the lazy restore leaves the virtual-map planes to the step: the panels are then two thirds
// of a restore's bytes - 11.9 against 12.3 us per restore with four parts, 13.2 with sixteen; profiles/lazy_restore_ab.txt)
constexpr int kCopySplit = 8;
// mode 1: header, jd and body.  mode 2 (a lazy restore): a valid panel's body stays in s - the header says so (kPanelInSrc) and the
// belief step that follows reads it there (k_inc.hip).  mode 3 (settling that debt): the bodies mode 2 left behind, and the header's
// valid word without the mark; s is a snapshot instance, which nothing writes, so its header still says which bodies those are.
__device__ __forceinline__ void copy_panel_part(const DrlgxState &S, int s, int d, int part, int mode) {
  const int *ms = S.jc_meta + (size_t)s * 4;
  int *md = S.jc_meta + (size_t)d * 4;
  const int valid = ms[0] & ~kPanelInSrc, P = ms[1], L = ms[2], M = ms[3];
  if (threadIdx.x == 0 && part == 0) {
    if (mode != 3) {
      md[0] = (mode == 2 && valid == 1) ? (valid | kPanelInSrc) : valid; md[1] = P; md[2] = L; md[3] = M;
    } else if (valid == 1) {
      md[0] = valid;
    }
  }
  if (valid != 1) return;
  if (mode != 2) drlgx_copy_panel_body<256>(S.jc, S.jc_stride, S.jc_ld, S.P_max, s, d, P, L, part, kCopySplit, threadIdx.x);
  if (part == 0 && mode != 3)
    for (int e = threadIdx.x; e < 6 * P; e += 256) S.jd[(size_t)d * S.P_max * 6 + e] = S.jd[(size_t)s * S.P_max * 6 + e];
}

// copy every field of instance src[i] to dst[i] whose class is not in skip_mask (and is only_cls, if that is >= 0) and - panel
// != 0: copy_panel_part's mode - its covariance panel: one launch for everything an instance copy (snapshot / restore, env -> base -> rollout) moves
__global__ __launch_bounds__(256) void k_copy_instances(const DrlgxField *fields, int n_fields, const int32_t *src,
                                                        const int32_t *dst, int src_off, int dst_off, int skip_mask, int only_cls,
                                                        const int *cnt, DrlgxState S, int panel) {
  // grid = (instances, fields [+ kCopySplit]): every (instance, field) slice is streamed by its own workgroup with
  // 16-byte accesses when the slice is 16-byte aligned (all large fields are)
  // (x = field, y = instance: consecutive workgroups stream slices of DIFFERENT arrays - with x = instance the workgroups in flight
  // all walked the same field at the same offsets of 256 instances: 20.8 against 18.0 us per 78 MB restore, profiles/r06_ab_copy.txt)
  // (a 1-D grid dealt so that instance i's slices are copied on XCD i % 8 - where the belief kernels' workgroup of instance i runs
  // next - changed neither kernel's time)
  const int i = blockIdx.y;
  const int f = blockIdx.x;
  const int s = (src ? src[i] : i) + src_off, d = (dst ? dst[i] : i) + dst_off;
  if (f >= n_fields) {
    if (panel) copy_panel_part(S, s, d, f - n_fields, panel);
    return;
  }
  // (one workgroup for ALL the fields of a few bytes per instance was measured: 21.4 against 17.8 us - seven dependent round trips)
  if ((fields[f].cls & skip_mask) || (only_cls >= 0 && fields[f].cls != only_cls)) return;
  const size_t stride = fields[f].stride;
  const char *sb = fields[f].base + (size_t)s * stride;
  char *db = fields[f].base + (size_t)d * stride;
  // the live part: per-pose / per-landmark / per-factor arrays end at the source instance's counts
  // (pad: a sub-slice of the instance's slice - one plane of the virtual map's information)
  const int unit = cnt ? fields[f].unit : 0;
  int count = 0;
  if (unit) {
    const int *c = cnt + (size_t)s * DRLGX_CNT_STRIDE;
    count = unit == 1 ? c[C_P] : unit == 2 ? c[C_L] : c[C_M];
  }
  const size_t live = drlgx_field_live_bytes(stride, unit, fields[f].unit_bytes, fields[f].pad, count);
  if (!drlgx_field_by_words(stride)) {
    const uint4 *sp = reinterpret_cast<const uint4 *>(sb);
    uint4 *dp = reinterpret_cast<uint4 *>(db);
    const size_t nq = live / 16;
    size_t k = threadIdx.x;
    for (; k + 256 < nq; k += 512) {  // (two loads in flight per thread)
      const uint4 v0 = sp[k], v1 = sp[k + 256];
      dp[k] = v0; dp[k + 256] = v1;
    }
    if (k < nq) dp[k] = sp[k];
  } else {
    const uint32_t *sp = reinterpret_cast<const uint32_t *>(sb);
    uint32_t *dp = reinterpret_cast<uint32_t *>(db);
    const size_t nw = (live < stride ? live : stride) / 4;
    for (size_t k = threadIdx.x; k < nw; k += 256) dp[k] = sp[k];
  }
}

// A lazy restore (snapshot instance src_off + i -> env i: k_copy_instances with skip_mask 1 and copy_panel_part's mode 2) by ONE
// workgroup per env.  The generic kernel's grid is (31 fields + 8 panel parts) x envs - about 10 000 workgroups at 256 envs, most of
// which return at once or move a few bytes behind two dependent reads - for the 23 KB per env a lazy restore still moves at the
// bench state.  Here the first wave reads the source's counts, its panel header and the table (drlgx_restore_table: n_tab <=
// kRestoreMaxEntries entries, the first n16 moved as 16-byte items, the others as words) in one round trip, lane k computes entry k's
// live items (drlgx_field_live_bytes: the byte ranges are the generic kernel's) and a wave scan leaves their prefix in LDS.  The items
// of all entries form one index space; thread t serves items t, t + T, ... of either kind, finds (entry, offset) by a five-step
// search of the prefix, and has kRestoreDepth + kRestoreWordDepth loads in flight before its first store.
constexpr int kRestoreDepth = 4, kRestoreWordDepth = 2;
#ifndef DRLGX_RESTORE_THREADS
// (headline, M env-steps/s: 256 threads 4.30-4.35, 512 threads 4.36-4.42, 1024 threads 4.43-4.46 in three runs - ahead of 512 by
// about one run's spread, not separated from it; the generic kernel 4.17-4.20; profiles/restore_compact_ab.txt)
#define DRLGX_RESTORE_THREADS 512
#endif
constexpr int kRestoreThreads = DRLGX_RESTORE_THREADS;

// (its slices are addressed as global memory, not through flat pointers read back from LDS: plain vector types in that address space)
typedef unsigned int restore_q __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) restore_q restore_gq;
typedef __attribute__((address_space(1))) uint32_t restore_gw;

// the entry that holds item i: the largest k with pre[k] <= i (empty entries share their successor's prefix; pre[n_tab ..] = all items)
__device__ __forceinline__ int restore_entry_of(const unsigned *pre, unsigned i) {
  int k = 0;
#pragma unroll
  for (int step = kRestoreMaxEntries / 2; step; step >>= 1)
    if (pre[k + step] <= i) k += step;
  return k;
}

template <int T>
__global__ __launch_bounds__(T) void k_restore_compact(const DrlgxField *__restrict__ tab, int n_tab, int n16, int src_off,
                                                       const int *__restrict__ cnt, int *jc_meta) {
  __shared__ unsigned pre[kRestoreMaxEntries + 1];  // pre[k]: items in front of entry k
  __shared__ uintptr_t src_of[kRestoreMaxEntries], dst_of[kRestoreMaxEntries];  // the instances' slices of entry k
  const int d = blockIdx.x, s = d + src_off, tid = threadIdx.x;
  if (tid < 64) {
    // one round trip: the lane's table entry, the source's counts and its panel header are requested together, by lane-indexed
    // loads that are handed round afterwards (left as uniform loads they are sunk into the branches that use them, each behind
    // the table's; an engine without panels reads the counts' row in the header's place - no branch between the loads)
    const DrlgxField f = tab[tid < n_tab ? tid : n_tab - 1];
    const int *c = cnt + (size_t)s * DRLGX_CNT_STRIDE;
    const int *ms = jc_meta ? jc_meta + (size_t)s * 4 : c;
    static_assert(DRLGX_CNT_STRIDE == 8, "the lanes read the counts' row by tid & 7");
    const int cv = c[tid & 7], hv = ms[tid & 3];
    const int cP = __shfl(cv, C_P), cL = __shfl(cv, C_L), cM = __shfl(cv, C_M);
    const int valid = jc_meta ? __shfl(hv, 0) & ~kPanelInSrc : 0, mP = __shfl(hv, 1), mL = __shfl(hv, 2), mM = __shfl(hv, 3);
    unsigned items = 0;
    if (tid < n_tab) {
      const int count = f.unit == 1 ? cP : f.unit == 2 ? cL : f.unit == 3 ? cM : valid == 1 ? mP : 0;
      items = (unsigned)drlgx_field_items(f.stride, drlgx_field_live_bytes(f.stride, f.unit, f.unit_bytes, f.pad, count));
      src_of[tid] = reinterpret_cast<uintptr_t>(f.base + (size_t)s * f.stride);
      dst_of[tid] = reinterpret_cast<uintptr_t>(f.base + (size_t)d * f.stride);
    }
    unsigned incl = items;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o);
      if (tid >= o) incl += up;
    }
    if (tid <= kRestoreMaxEntries) pre[tid] = incl - items;  // (lanes behind the table hold no items: their prefix is the total)
    if (tid == 0 && jc_meta) {  // copy_panel_part's mode 2: a valid panel's body stays in s, and the header says so
      int *md = jc_meta + (size_t)d * 4;
      md[0] = valid == 1 ? (valid | kPanelInSrc) : valid; md[1] = mP; md[2] = mL; md[3] = mM;
    }
  }
  __syncthreads();
  const unsigned N16 = pre[n16], N = pre[kRestoreMaxEntries];
  for (unsigned a = tid, b = N16 + tid; a < N16 || b < N; a += T * kRestoreDepth, b += T * kRestoreWordDepth) {
    // (the searches of a trip are independent and unguarded, so that their LDS reads overlap; the values stay in registers)
    int kv[kRestoreDepth], kw[kRestoreWordDepth];
#pragma unroll
    for (int j = 0; j < kRestoreDepth; ++j) kv[j] = restore_entry_of(pre, a + j * T);
#pragma unroll
    for (int j = 0; j < kRestoreWordDepth; ++j) kw[j] = restore_entry_of(pre, b + j * T);
    restore_q v[kRestoreDepth];
    restore_gq *vp[kRestoreDepth];
    uint32_t w[kRestoreWordDepth];
    restore_gw *wp[kRestoreWordDepth];
#pragma unroll
    for (int j = 0; j < kRestoreDepth; ++j) {
      const unsigned i = a + j * T;
      const size_t off = i - pre[kv[j]];
      const restore_gq *sp = (const restore_gq *)src_of[kv[j]] + off;
      vp[j] = (restore_gq *)dst_of[kv[j]] + off;
      v[j] = restore_q{0, 0, 0, 0};
      if (i < N16) v[j] = *sp;
    }
#pragma unroll
    for (int j = 0; j < kRestoreWordDepth; ++j) {
      const unsigned i = b + j * T;
      const size_t off = i - pre[kw[j]];
      const restore_gw *sp = (const restore_gw *)src_of[kw[j]] + off;
      wp[j] = (restore_gw *)dst_of[kw[j]] + off;
      w[j] = 0;
      if (i < N) w[j] = *sp;
    }
#pragma unroll
    for (int j = 0; j < kRestoreDepth; ++j)
      if (a + j * T < N16) *vp[j] = v[j];
#pragma unroll
    for (int j = 0; j < kRestoreWordDepth; ++j)
      if (b + j * T < N) *wp[j] = w[j];
  }
}

// What a status read brings to the host, packed for ONE copy: [status word, every env's pose count] (head bytes, a multiple of 16),
// then the caller's bytes (drlgx_status_fetch_host).  Separate copies - a word, a strided column of the counters, the caller's
// buffer - cost more in submission than this launch: 40 us per read on an idle stream against ~15 for a single copy.
__global__ __launch_bounds__(256) void k_fetch_pack(const int *status, const int *cnt, int n_envs, int head, const unsigned char *src,
                                                    size_t bytes, unsigned char *out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nt = (size_t)gridDim.x * 256;
  int *h = reinterpret_cast<int *>(out);
  for (size_t i = t; i < (size_t)n_envs + 1; i += nt) h[i] = i == 0 ? status[0] : cnt[(i - 1) * DRLGX_CNT_STRIDE + C_P];
  unsigned char *o = out + head;
  if (((reinterpret_cast<uintptr_t>(src) | bytes) & 15) == 0) {
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *o4 = reinterpret_cast<uint4 *>(o);
    for (size_t i = t; i < bytes / 16; i += nt) o4[i] = s4[i];
  } else {
    for (size_t i = t; i < bytes; i += nt) o[i] = src[i];
  }
}

// SLAM2D::set_copy_isam: theta := calculateBestEstimate(), delta := 0, fresh ISAM2 (update count 0)
__global__ __launch_bounds__(64) void k_rebase(DrlgxState S, int base0, int n) {
  const int inst = base0 + blockIdx.x;
  int *cnt = S.cnt + (size_t)inst * DRLGX_CNT_STRIDE;
  const int P = cnt[C_P], L = cnt[C_L];
  for (int i = threadIdx.x; i < P; i += 64) {
    for (int k = 0; k < 4; ++k)
      S.th_pose[((size_t)inst * S.P_max + i) * 4 + k] = S.est_pose[((size_t)inst * S.P_max + i) * 4 + k];
    for (int k = 0; k < 3; ++k) S.d_pose[((size_t)inst * S.P_max + i) * 3 + k] = 0.0;
  }
  for (int j = threadIdx.x; j < L; j += 64) {
    for (int k = 0; k < 2; ++k) {
      S.th_lm[((size_t)inst * S.L_max + j) * 2 + k] = S.est_lm[((size_t)inst * S.L_max + j) * 2 + k];
      S.d_lm[((size_t)inst * S.L_max + j) * 2 + k] = 0.0;
    }
  }
  if (threadIdx.x == 0) {
    cnt[C_ISAM] = 0;
    cnt[C_NEWP] = 0;
    cnt[C_NEWL] = 0;
    cnt[C_FLAG] = 0;
    if (S.jc_meta) S.jc_meta[(size_t)inst * 4] = 0;  // the re-based system is solved in full (and leaves a fresh covariance panel)
  }
}

// after copying base -> rollout: result_ (est_pose) is the ORIGINAL estimate of the live env
// (SLAM2D copy keeps result_; set_copy_isam does not touch it), distance accumulator reset.
__global__ __launch_bounds__(64) void k_fix_rollouts(DrlgxState S, const int32_t *cand_env, int roll0) {
  const int c = blockIdx.x;
  const int env = cand_env[c], inst = roll0 + c;
  const int P = S.cnt[(size_t)inst * DRLGX_CNT_STRIDE + C_P];
  for (int e = threadIdx.x; e < P * 4; e += 64)
    S.est_pose[(size_t)inst * S.P_max * 4 + e] = S.est_pose[(size_t)env * S.P_max * 4 + e];
  if (threadIdx.x == 0) {
    S.parent[inst] = env;
    S.red[(size_t)inst * DRLGX_RED_STRIDE + R_DIST] = 0.0;
  }
}

__device__ __forceinline__ double utility_of(const DrlgxState &S, int inst, double dist) {
  const double *red = S.red + (size_t)inst * DRLGX_RED_STRIDE;
  const drlgx_config &cfg = S.cfg;
  const double pk = red[R_KNOWN] / (double)S.V;
  const double dw = cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * pk;
  return red[R_UTR] + dist * dw;
}

__global__ void k_rewards(DrlgxState S, int n_cand, const int32_t *cand_env, int roll0, double *rewards) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cand) return;
  const int inst = roll0 + c;
  const double u0 = utility_of(S, cand_env[c], 0.0);
  const double u1 = utility_of(S, inst, S.red[(size_t)inst * DRLGX_RED_STRIDE + R_DIST]);
  rewards[c] = u0 - u1;
}

// mode 0: calculateUtility(dist); 1: explored(); 2: uncertainty_EM trace-weighted; 3: uncertainty_EM det
__global__ void k_utility(DrlgxState S, const double *dist, double *out, int mode) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S.n_envs) return;
  const double *red = S.red + (size_t)e * DRLGX_RED_STRIDE;
  if (mode == 0) out[e] = utility_of(S, e, dist ? dist[e] : 0.0);
  else if (mode == 1) out[e] = red[R_EXPL] / (double)S.count_explored;
  else if (mode == 2) out[e] = red[R_UWTR];
  else out[e] = red[R_UDET];
}

// EMPlanner2D::line_planner (Planner2D.cpp:937-1041), goal = frontier point
__global__ void k_line_plan(DrlgxState S, int n_cand, const int32_t *cand_env, const double *goal, double *actions,
                            int32_t *n_actions) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cand) return;
  const int env = cand_env[c];
  const int P = S.cnt[(size_t)env * DRLGX_CNT_STRIDE + C_P];
  const double *ep = S.est_pose + ((size_t)env * S.P_max + (P - 1)) * 4;
  const double rx = ep[0], ry = ep[1];
  double rth = atan2(ep[3], ep[2]);
  const double gx = goal[2 * c], gy = goal[2 * c + 1];
  double gth = atan2(gy - ry, gx - rx);
  const double PI = 3.14159265358979323846;
  if (rth < 0) rth = PI * 2 + rth;
  if (gth < 0) gth = PI * 2 + gth;
  const double dr = 180 * PI / 180;
  double diff = gth - rth;
  double *out = actions + (size_t)c * S.A_max * 3;
  int n = 0;
  double d, sign;
  if (diff > PI) {
    d = 2 * PI - diff;
    sign = -1.0;
  } else if (diff > -PI && diff < 0) {
    d = fabs(diff);
    sign = -1.0;
  } else if (diff <= -PI) {
    d = 2 * PI - fabs(diff);
    sign = 1.0;
  } else {
    d = diff;
    sign = 1.0;
  }
  auto push = [&](double x, double y, double th) {
    if (n < S.A_max) {
      // a Pose2 action: theta() = atan2(sin, cos)
      out[3 * n] = x;
      out[3 * n + 1] = y;
      out[3 * n + 2] = atan2(sin(th), cos(th));
    }
    n++;
  };
  {
    const int q = (int)(d / dr);
    const double rem = d - dr * q;
    for (int i = 0; i < q; ++i) push(0, 0, sign * dr);
    push(0, 0, sign * rem);
  }
  const double dist = sqrt(pow(rx - gx, 2) + pow(ry - gy, 2));
  const int dq = (int)(dist / S.cfg.max_edge_length);
  const double drem = dist - dq * S.cfg.max_edge_length;
  for (int i = 0; i < dq; ++i) push(S.cfg.max_edge_length, 0, 0);
  push(drem, 0, 0);
  n_actions[c] = n;
  if (n > S.A_max) atomicMin(S.status, DRLGX_E_CAPACITY);
}

// The metric trio of the reference's evaluation script for environment e, by one 256-thread workgroup (red: its 3 x 4 doubles of
// LDS); thread 0 returns with the values in m[0..2], the other threads' m is undefined:
//   m[0] landmark error   (exploration_env.py:170-177): (sum_j |gt[key_j] - est_j| + sigma0 (n_gt - L)) / n_gt
//   m[1] map entropy      (scripts/test.py:61-74): -sum_v p ln p + 0.5 ln(0.5) (V - interior cells)
//   m[2] max localisation uncertainty (exploration_env.py:190-194): max over the poses of tr(marginal covariance)
// k_metrics and k_plan_record both call it: one reduction order, the same bits.
__device__ __forceinline__ void metrics_of(const DrlgxState &S, int e, double sigma0, double (*red)[4], double (&m)[3]) {
  const int tid = threadIdx.x;
  const int *cnt = S.cnt + (size_t)e * DRLGX_CNT_STRIDE;
  const int P = cnt[C_P], L = cnt[C_L];
  const double *gt = S.gt_lm + (size_t)S.parent[e] * S.LG * 2;
  const double *el = S.est_lm + (size_t)e * S.L_max * 2;
  const int *key = S.lm_key + (size_t)e * S.L_max;
  double err = 0, ent = 0, mx = 0;
  for (int j = tid; j < L; j += 256) {
    const double dx = gt[2 * key[j]] - el[2 * j], dy = gt[2 * key[j] + 1] - el[2 * j + 1];
    err += sqrt(dx * dx + dy * dy);
  }
  const double *prob = S.vm_prob + (size_t)e * S.V;
  for (int v = tid; v < S.V; v += 256) ent += prob[v] * log(prob[v]);
  const double *ptr = S.pose_tr + (size_t)e * S.P_max;
  for (int i = tid; i < P; i += 256) mx = fmax(mx, ptr[i]);
  for (int o = 32; o > 0; o >>= 1) {
    err += __shfl_down(err, o);
    ent += __shfl_down(ent, o);
    mx = fmax(mx, __shfl_down(mx, o));
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = err;
    red[1][tid >> 6] = ent;
    red[2][tid >> 6] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    const int n_gt = S.cfg.num_landmarks;
    const double es = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const double hs = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    m[0] = (es + sigma0 * (n_gt - L)) / n_gt;
    m[1] = -hs + 0.5 * log(0.5) * (double)(S.V - S.count_explored);
    m[2] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
  }
}

// out[3 e + 0 .. 2] = the trio of every environment, one workgroup each
__global__ __launch_bounds__(256) void k_metrics(DrlgxState S, double sigma0, double *out) {
  __shared__ double red[3][4];
  const int e = blockIdx.x;
  double m[3];
  metrics_of(S, e, sigma0, red, m);
  if (threadIdx.x == 0) {
    out[3 * e] = m[0];
    out[3 * e + 1] = m[1];
    out[3 * e + 2] = m[2];
  }
}

// The evaluation loop's per-action record (scripts/test.py:128-152), launched behind action index a of the chosen plans, one
// workgroup per environment; an env whose plan has ended (a >= n_actions[e]) is left alone.  trace[e][a] = (the trio of k_metrics,
// VirtualMap::explored as k_utility's mode 1 computes it), then ExplorationEnv.step's terminal test (exploration_env.py:107-110):
// when it holds the env is flagged done and its plan is cut behind this action, so that the launches of the later action indices
// skip it (LaunchSel::on reads n_actions).
__global__ __launch_bounds__(256) void k_plan_record(DrlgxState S, double sigma0, int a, int32_t *n_actions, double done_explored,
                                                     int max_steps, double *trace, int32_t *done) {
  __shared__ double red[3][4];
  const int e = blockIdx.x;
  if (a >= n_actions[e]) return;  // (the whole workgroup: nobody waits at metrics_of's barrier)
  double m[3];
  metrics_of(S, e, sigma0, red, m);
  if (threadIdx.x == 0) {
    double *t = trace + ((size_t)e * S.A_max + a) * 4;
    const double explored = S.red[(size_t)e * DRLGX_RED_STRIDE + R_EXPL] / (double)S.count_explored;
    t[0] = m[0];
    t[1] = m[1];
    t[2] = m[2];
    t[3] = explored;
    if (explored > done_explored || S.cnt[(size_t)e * DRLGX_CNT_STRIDE + C_STEP] > max_steps) {
      done[e] = 1;
      n_actions[e] = a + 1;
    }
  }
}

// ---- following a plan (EMExplorer.follow_path and explore()'s result switch, scripts/envs/pyplanner2d.py:100-109,170-187) ----
// SS2D.simulate's bounds test of an odometry increment (pyss2d.py:173-176) - ksim::odom_in_bounds (k_sim.hip) restated for this unit
__device__ __forceinline__ bool follow_odom_ok(const drlgx_config &cfg, const double *a) {
  return (cfg.map_min_x < a[0] && a[0] < cfg.map_max_x) && (cfg.map_min_y < a[1] && a[1] < cfg.map_max_y);
}

// What every env executes, one wave per env: SUCCESS (3) the first min(steps, n_actions) rows of its plan, SAMPLING_FAILURE (0)
// the fallback move, anything else - or an inactive env - nothing (stop 4 / 5 for NO_SOLUTION / TERMINATION, else 0).  A first
// action outside the map box is a rejected odometry before anything ran: no action, stop 3.
__global__ __launch_bounds__(64) void k_follow_select(DrlgxState S, const double *plan, const int32_t *n_actions, const int32_t *result,
                                                      const uint8_t *active, int steps, double fx, double fy, double fth, double *act,
                                                      int32_t *n_exec, int32_t *stop) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int res = result[e];
  const bool on = !active || active[e];
  int n = 0;
  if (on && res == 3) n = min(min(max(steps, 0), max(n_actions[e], 0)), S.A_max);
  else if (on && res == 0) n = 1;
  const double *src = plan + (size_t)e * S.A_max * 3;
  double *dst = act + (size_t)e * S.A_max * 3;
  const double fb[3] = {fx, fy, fth};
  for (int k = lane; k < 3 * S.A_max; k += 64) dst[k] = k >= 3 * n ? 0.0 : res == 0 ? fb[k] : src[k];
  if (lane == 0) {
    const double first[3] = {res == 0 ? fx : src[0], res == 0 ? fy : src[1], 0.0};
    const bool rejected = n > 0 && !follow_odom_ok(S.cfg, first);
    n_exec[e] = rejected ? 0 : n;
    stop[e] = rejected ? 3 : res == 1 ? 4 : res == 2 ? 5 : 0;
  }
}

// k_plan_record for a followed plan: the same row and the same `done` cut (stop 1), then the two cuts of follow_path - the step
// raised the obstacle flag (red[R_OBS], written under drlgx_set_env_obstacles only: stop 2, the step itself stays executed and
// recorded), or the env's NEXT action is a rejected odometry (stop 3: it is never launched) - each by cutting n_exec behind this action.
__global__ __launch_bounds__(256) void k_follow_record(DrlgxState S, double sigma0, int a, const double *act, int32_t *n_exec,
                                                       int obstacles, double done_explored, int max_steps, double *trace, int32_t *done, int32_t *stop) {
  __shared__ double red[3][4];
  const int e = blockIdx.x;
  if (a >= n_exec[e]) return;  // (the whole workgroup: nobody waits at metrics_of's barrier)
  double m[3];
  metrics_of(S, e, sigma0, red, m);
  if (threadIdx.x == 0) {
    double *t = trace + ((size_t)e * S.A_max + a) * 4;
    const double explored = S.red[(size_t)e * DRLGX_RED_STRIDE + R_EXPL] / (double)S.count_explored;
    t[0] = m[0];
    t[1] = m[1];
    t[2] = m[2];
    t[3] = explored;
    int why = 0;
    if (explored > done_explored || S.cnt[(size_t)e * DRLGX_CNT_STRIDE + C_STEP] > max_steps) {
      done[e] = 1;
      why = 1;
    } else if (obstacles && S.red[(size_t)e * DRLGX_RED_STRIDE + R_OBS] != 0.0) {
      why = 2;
    } else if (a + 1 < n_exec[e] && !follow_odom_ok(S.cfg, act + ((size_t)e * S.A_max + a + 1) * 3)) {
      why = 3;
    }
    if (why) {
      n_exec[e] = a + 1;
      stop[e] = why;
    }
  }
}

// out[e] = the last step's obstacle flag, out[n_envs + e] = the cleared latch (pyss2d.py:132,183-197)
__global__ void k_obstacle_flags(DrlgxState S, uint8_t *out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S.n_envs) return;
  const double *red = S.red + (size_t)e * DRLGX_RED_STRIDE;
  out[e] = red[R_OBS] != 0.0 ? 1 : 0;
  out[S.n_envs + e] = red[R_LATCH] != 0.0 ? 0 : 1;
}

// numpy's arg-max order over (value, index) pairs: a NaN beats every number, among equals (and among NaNs) the lower index wins;
// index < 0 = no element
__device__ __forceinline__ bool pick_beats(float v, int i, float bv, int bi) {
  if (i < 0) return false;
  if (bi < 0) return true;
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// The greedy decision of the evaluation loop (scripts/test.py:110-119), one wave per environment: choice[e] = np.argmax over the
// env's frontier segment score[seg_begin[e] .. + n_frontier[e]) and the line plan of that frontier slot out of the padded plans of
// Engine.graph(plan=True), zero-filled behind its length.  An inactive env or one without frontiers: choice -1, an empty plan.
// Lanes stride over the segment, then a butterfly over (value, index): registers only.
__global__ __launch_bounds__(64) void k_greedy_plans(const float *score, int n_score, const int32_t *seg_begin, const int32_t *n_frontier,
                                                     const uint8_t *active, const double *actions_pad, const int32_t *n_act_pad,
                                                     int max_frontier, int max_actions, int32_t *choice, double *actions_out,
                                                     int32_t *n_actions_out) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int b = seg_begin[e];
  // (a segment that is not inside score[0, n_score) is a caller's error: it is cut there instead of read)
  const int n = (active && !active[e]) || b < 0 ? 0 : min(min(n_frontier[e], max_frontier), n_score - b);
  const float *q = score + b;
  float bv = 0.f;
  int bi = -1;
  for (int i = lane; i < n; i += 64) {
    const float v = q[i];
    if (pick_beats(v, i, bv, bi)) { bv = v; bi = i; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (pick_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  int na = 0;
  const double *src = actions_pad;
  if (bi >= 0) {
    const size_t slot = (size_t)e * max_frontier + bi;
    na = min(max(n_act_pad[slot], 0), max_actions);
    src += slot * max_actions * 3;
  }
  double *dst = actions_out + (size_t)e * max_actions * 3;
  for (int k = lane; k < 3 * max_actions; k += 64) dst[k] = k < 3 * na ? src[k] : 0.0;
  if (lane == 0) {
    choice[e] = bi;
    n_actions_out[e] = na;
  }
}

// VirtualMap::toCovArray (VirtualMap.cpp:140-151): per cell the larger eigenvalue of the 2x2 covariance (its square
// root clipped at sigma0) and the direction of its eigenvector.  Eigen's SelfAdjointEigenSolver returns a rotation
// (cos > 0) with the columns sorted by eigenvalue, so the eigenvector's sign is fixed by: x component > 0 when the
// larger eigenvalue belongs to the first axis, y component > 0 otherwise (recalled from Eigen; used for rendering only).
__global__ __launch_bounds__(256) void k_cov_array(DrlgxState S, double *length, double *angle) {
  const int e = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
  if (v >= S.V) return;
  const double *inf = S.vm_info + (size_t)e * 3 * S.V;
  double a, b, d;
  inv2_llt_s(inf[v], inf[S.V + v], inf[2 * S.V + v], a, b, d);  // covariance()
  const double half = 0.5 * (a - d), r = sqrt(half * half + b * b);
  const double lmax = 0.5 * (a + d) + r;
  double vx, vy;
  if (a >= d) {  // (lmax - d, b) is parallel to the eigenvector and its x component is >= 0
    vx = half + r; vy = b;
    if (vx == 0.0 && vy == 0.0) { vx = 1.0; vy = 0.0; }
  } else {       // (b, lmax - a): y component >= 0
    vx = b; vy = r - half;
  }
  length[(size_t)e * S.V + v] = fmin(sqrt(lmax), S.cfg.sigma0);
  angle[(size_t)e * S.V + v] = atan2(vy, vx);
}

}  // namespace

void drlgx_launch_metrics(const DrlgxState &S, hipStream_t st, double sigma0, double *out) {
  hipLaunchKernelGGL(k_metrics, dim3(S.n_envs), dim3(256), 0, st, S, sigma0, out);
}
void drlgx_launch_plan_record(const DrlgxState &S, hipStream_t st, double sigma0, int a, int32_t *n_actions, double done_explored,
                              int max_steps, double *trace, int32_t *done) {
  hipLaunchKernelGGL(k_plan_record, dim3(S.n_envs), dim3(256), 0, st, S, sigma0, a, n_actions, done_explored, max_steps, trace, done);
}
void drlgx_launch_follow_select(const DrlgxState &S, hipStream_t st, const double *plan, const int32_t *n_actions, const int32_t *result,
                                const uint8_t *active, int steps, const double *fallback, double *act, int32_t *n_exec, int32_t *stop) {
  hipLaunchKernelGGL(k_follow_select, dim3(S.n_envs), dim3(64), 0, st, S, plan, n_actions, result, active, steps, fallback[0], fallback[1],
                     fallback[2], act, n_exec, stop);
}
void drlgx_launch_follow_record(const DrlgxState &S, hipStream_t st, double sigma0, int a, const double *act, int32_t *n_exec, int obstacles,
                                double done_explored, int max_steps, double *trace, int32_t *done, int32_t *stop) {
  hipLaunchKernelGGL(k_follow_record, dim3(S.n_envs), dim3(256), 0, st, S, sigma0, a, act, n_exec, obstacles, done_explored, max_steps, trace,
                     done, stop);
}
void drlgx_launch_obstacle_flags(const DrlgxState &S, hipStream_t st, uint8_t *out) {
  hipLaunchKernelGGL(k_obstacle_flags, dim3((S.n_envs + 127) / 128), dim3(128), 0, st, S, out);
}
void drlgx_launch_cov_array(const DrlgxState &S, hipStream_t st, double *length, double *angle) {
  hipLaunchKernelGGL(k_cov_array, dim3((S.V + 255) / 256, S.n_envs), dim3(256), 0, st, S, length, angle);
}
void drlgx_launch_copy(const DrlgxField *fields_dev, int n_fields, hipStream_t st, int n, const int32_t *src,
                       const int32_t *dst, int src_off, int dst_off, int skip_mask, const int *cnt, const DrlgxState *panel,
                       int only_cls, int panel_mode) {
  if (n <= 0) return;
  const bool with_panel = panel && panel->jc;
  const dim3 cgrid(n_fields + (with_panel ? kCopySplit : 0), n);
  hipLaunchKernelGGL(k_copy_instances, cgrid, dim3(256), 0, st, fields_dev, n_fields, src, dst,
                     src_off, dst_off, skip_mask, only_cls, cnt, with_panel ? *panel : DrlgxState{}, with_panel ? panel_mode : 0);
}
void drlgx_launch_restore_compact(const DrlgxField *tab_dev, int n_tab, int n16, hipStream_t st, int n, int src_off, const int *cnt,
                                  int *jc_meta) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_restore_compact<kRestoreThreads>, dim3(n), dim3(kRestoreThreads), 0, st, tab_dev, n_tab, n16, src_off, cnt, jc_meta);
}
int drlgx_restore_items_per_trip() { return kRestoreThreads * kRestoreDepth; }
void drlgx_launch_fetch_pack(const DrlgxState &S, hipStream_t st, const void *src, size_t bytes, void *out) {
  const size_t head = drlgx_fetch_head_bytes(S.n_envs);
  const int blocks = (int)std::min<size_t>(256, (head + bytes + 4095) / 4096);
  hipLaunchKernelGGL(k_fetch_pack, dim3(std::max(blocks, 1)), dim3(256), 0, st, S.status, S.cnt, S.n_envs, (int)head,
                     reinterpret_cast<const unsigned char *>(src), bytes, reinterpret_cast<unsigned char *>(out));
}
void drlgx_launch_rebase(const DrlgxState &S, hipStream_t st, int base0, int n) {
  hipLaunchKernelGGL(k_rebase, dim3(n), dim3(64), 0, st, S, base0, n);
}
void drlgx_launch_fix_rollouts(const DrlgxState &S, hipStream_t st, int n_cand, const int32_t *cand_env, int roll0) {
  hipLaunchKernelGGL(k_fix_rollouts, dim3(n_cand), dim3(64), 0, st, S, cand_env, roll0);
}
void drlgx_launch_rewards(const DrlgxState &S, hipStream_t st, int n_cand, const int32_t *cand_env, int roll0,
                          double *rewards) {
  hipLaunchKernelGGL(k_rewards, dim3((n_cand + 127) / 128), dim3(128), 0, st, S, n_cand, cand_env, roll0, rewards);
}
void drlgx_launch_utility(const DrlgxState &S, hipStream_t st, const double *dist, double *out, int mode) {
  hipLaunchKernelGGL(k_utility, dim3((S.n_envs + 127) / 128), dim3(128), 0, st, S, dist, out, mode);
}
void drlgx_launch_line_plan(const DrlgxState &S, hipStream_t st, int n_cand, const int32_t *cand_env, const double *goal,
                            double *actions, int32_t *n_actions) {
  hipLaunchKernelGGL(k_line_plan, dim3((n_cand + 127) / 128), dim3(128), 0, st, S, n_cand, cand_env, goal, actions,
                     n_actions);
}

int drlgx_greedy_plans(void *hip_stream, int n_envs, const float *score, int n_score, const int32_t *seg_begin, const int32_t *n_frontier,
                       const uint8_t *active, const double *actions_pad, const int32_t *n_act_pad, int max_frontier, int max_actions,
                       int32_t *choice, double *actions_out, int32_t *n_actions_out) {
  if (n_envs <= 0 || !score || n_score < 0 || !seg_begin || !n_frontier || !actions_pad || !n_act_pad || max_frontier <= 0 || max_actions <= 0 ||
      !choice || !actions_out || !n_actions_out)
    return DRLGX_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL(k_greedy_plans, dim3(n_envs), dim3(64), 0, st, score, n_score, seg_begin, n_frontier, active, actions_pad, n_act_pad,
                     max_frontier, max_actions, choice, actions_out, n_actions_out);
  return hipGetLastError() == hipSuccess ? DRLGX_OK : DRLGX_E_HIP;
}
