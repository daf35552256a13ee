// Host side of the SLAM stage: what the dense solver (k_slam.hip) needs in LDS for given capacities - the pose-chain solver's
// LDS and workspace layout is arrow_carve.h -, which of the kernels serves an engine, and the launch of the stand-alone SLAM stage (called by drlgx_engine.cpp and
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
  return kslam::ArrowCarve::min_bytes(P_max, L_max) <= (size_t)kslam::kLdsBudget;
}
// doubles of HBM workspace per instance of the pose-chain solver; the dense solver's overflow (factor records, observation
// table) lies at its start.  The layout: arrow_carve.h
size_t drlgx_slam_ws_doubles(int P_max, int L_max, int M_max) { return kslam::ArrowWs(P_max, L_max, M_max).total; }

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
