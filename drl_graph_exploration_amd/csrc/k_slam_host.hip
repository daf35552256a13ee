// Host side of the SLAM stage: what the kernels of k_slam.hip / k_slam_arrow.hip need in LDS and workspace for given
// capacities, which of them serves an engine, and the launch of the stand-alone SLAM stage (called by drlgx_engine.cpp and
// by the host functions of k_step.hip).
#pragma once
#include <algorithm>
#include "k_slam.hip"
#include "k_slam_arrow.hip"
namespace kslam {
// LDS needed by the always-resident small arrays of the fast path
size_t slam_dim(int P_max) { return 16 * (((size_t)3 * P_max + 1 + 15) / 16); }
size_t slam_small_bytes(int P_max, int L_max, int M_max) {  // (SlamCtx::setup)
  return (size_t)P_max * 64 + (size_t)L_max * 16 + (size_t)L_max * 64 + (size_t)L_max * 8 * ((P_max + 63) / 64) +
         (size_t)(P_max + 2) * 4 + (size_t)(L_max + 2) * 8 + (size_t)M_max * 7 + (size_t)L_max * 2 + 224;
}
// LDS the arrow path cannot do without at full capacity: tables + the packed landmark system or the panels of the
// workspace variant (factor records and the observation table overflow to the workspace)
size_t arrow_lds_bytes(int P_max, int L_max, int M_max) {
  const size_t N = 16 * (((size_t)2 * L_max + 1 + 15) / 16);
  const size_t Tn = N / 16;
  // packed in LDS; register tiles + panels in LDS; or everything streamed from the workspace (E tiles + scratch in LDS)
  const size_t sys = N <= 16 * kFastTilesArrow ? sweep_region_doubles(N)
                     : Tn * (Tn + 1) / 2 <= (size_t)kArrowRegTiles * (kWaves - 1) ? 32 * N + 1280 : 1280;
  return arrow_small_bytes(P_max, L_max, M_max) + sys * 8 + 64;
}

}  // namespace kslam

// true when the fused LDS-resident kernel applies to trajectories of up to P_max poses
bool drlgx_slam_in_lds(int P_max, int L_max, int M_max) {
  const size_t n = kslam::slam_dim(P_max), nf = std::max<size_t>(n, 16 * kslam::kFastTiles);
  return n <= (size_t)16 * kslam::kDenseTiles &&
         kslam::slam_small_bytes(P_max, L_max, M_max) + kslam::sweep_region_doubles(nf) * 8 <= (size_t)kslam::kLdsBudget;
}
// capacities the SLAM kernels can serve at all (checked by drlgx_create)
bool drlgx_slam_capacity_ok(int P_max, int L_max, int M_max) {
  // (any number of landmarks: beyond the register-tile sweep the landmark system is streamed from the workspace)
  return kslam::arrow_lds_bytes(P_max, L_max, M_max) <= (size_t)kslam::kLdsBudget;
}
// doubles of HBM workspace per instance: X (3 P x (2 L + 1), row stride rounded up to 4), the selected-inverse blocks of the
// chain (6 + 9 + 9 per pose), the leaf -> right-separator rhs scratch, the square landmark system of the workspace variant, the factor records and the observation
// table when they do not fit the LDS
size_t drlgx_slam_ws_doubles(int P_max, int L_max, int M_max) {
  const size_t ldx = (size_t)((2 * L_max + 1 + 3 + 3) & ~3);  // (+ the three unit columns of the newest pose: arrow_body)
  const size_t n = (size_t)3 * P_max * ldx + (size_t)24 * P_max + (size_t)(P_max / kslam::kSeg + 2) * 3 * ldx + (size_t)(2 * L_max + 17) * (2 * L_max + 17) + (size_t)32 * (2 * L_max + 17) +
                   (size_t)M_max * kslam::REC + ((size_t)L_max * P_max * 2 + 7) / 8 + 16;
  return (n + 31) & ~(size_t)31;  // instances stay 256-byte aligned: 32-byte row loads of X
}

void drlgx_launch_slam(const DrlgxState &S, hipStream_t st, LaunchSel sel, int p_bound) {
  const int Pb = p_bound < S.P_max ? p_bound : S.P_max;
  if (sel.pcap <= 0) sel.pcap = Pb;
  static bool attr_set[32] = {false};
  const void *fns[] = {reinterpret_cast<const void *>(&kslam::k_slam<kslam::kFastTiles>),
                       reinterpret_cast<const void *>(&kslam::k_slam_arrow<0>),
                       reinterpret_cast<const void *>(&kslam::k_slam_arrow<kslam::kArrowRegTiles>)};
  drlgx_ensure_lds_attr(attr_set, fns, 3, kslam::kLdsBudget);
  const dim3 grid(sel.n), block(kslam::kThreads);
  // (the whole LDS is requested: what the tables and the system leave free holds the factor records and the observation table)
  if (drlgx_slam_in_lds(Pb, S.L_max, S.M_max))
    hipLaunchKernelGGL((kslam::k_slam<kslam::kFastTiles>), grid, block, kslam::kLdsBudget, st, DRLGX_KS_ARG(S), sel, kslam::kLdsBudget);
  else if (2 * S.L_max + 1 <= 16 * kslam::kFastTilesArrow)  // landmark system always packed in LDS: no register-tile sweep compiled in
    hipLaunchKernelGGL((kslam::k_slam_arrow<0>), grid, block, kslam::kLdsBudget, st, DRLGX_KS_ARG(S), sel, kslam::kLdsBudget);
  else
    hipLaunchKernelGGL((kslam::k_slam_arrow<kslam::kArrowRegTiles>), grid, block, kslam::kLdsBudget, st, DRLGX_KS_ARG(S), sel, kslam::kLdsBudget);
}
