// Host side of the SLAM stage: which capacities the dense solver (k_slam.hip; its LDS layout: slam_carve.h) and the pose-chain
// solver (LDS and workspace layout: arrow_carve.h) serve, which of the kernels serves an engine, and the launch of the stand-alone SLAM stage (called by drlgx_engine.cpp and
// by the host functions of k_step.hip).
#pragma once
#include <algorithm>
#include "k_slam.hip"
#include "k_slam_arrow.hip"
// true when the fused LDS-resident kernel applies to trajectories of up to P_max poses
bool drlgx_slam_in_lds(int P_max, int L_max, int M_max) {
  return kslam::SlamCarve::fits(P_max, L_max, M_max, 0, kslam::kLdsBudget);
}
// capacities the SLAM kernels can serve at all (checked by drlgx_create)
bool drlgx_slam_capacity_ok(int P_max, int L_max, int M_max) {
  // (any number of landmarks: beyond the register-tile sweep the landmark system is streamed from the workspace)
  return kslam::ArrowCarve::min_bytes(P_max, L_max) <= (size_t)kslam::kLdsBudget;
}
// doubles of HBM workspace per instance of the pose-chain solver; the dense solver's overflow (factor records, observation
// table) lies at its start.  The layout: arrow_carve.h
size_t drlgx_slam_ws_doubles(int P_max, int L_max, int M_max) { return kslam::ArrowWs(P_max, L_max, M_max).total; }

// register tiles per wave of the pose-chain kernel that serves an engine of up to L_max landmarks (0: its landmark system is
// always packed in LDS, no register-tile sweep compiled in)
static int arrow_ntw(int L_max) { return 2 * L_max + 1 <= 16 * kslam::kFastTilesArrow ? 0 : kslam::kArrowRegTiles; }

int drlgx_debug_arrow_form(int P, int L, int M, int L_max, int mk_panel, int32_t out[DRLGX_ARROW_FORM_N]) {
  if (!out || P < 1 || L < 0 || M < 0 || L > L_max || P > 65535 || L_max > 32767 || M > (1 << 24)) return DRLGX_E_INVALID;
  const int NTW = arrow_ntw(L_max);
  const kslam::ArrowCarve ac(P, L, M, NTW, kslam::kLdsBudget, mk_panel != 0);
  if (!ac.c_lds && NTW == 0) return DRLGX_E_INVALID;  // (ArrowCtx::setup leaves there)
  const int nK = (ac.np + 15) / 16, zfit = kslam::arrow_zfit(ac.u_free, nK > 0 ? nK : 1);
  out[0] = ac.c_lds ? 0 : ac.c_reg ? 1 : 2;
  out[1] = ac.obs_lds; out[2] = ac.xs_lds; out[3] = ac.rec_lds;
  out[4] = kslam::arrow_products_vector(ac.c_lds, ac.np) ? 0 : kslam::arrow_products_tiles(ac.np) ? 1 : 2;
  out[5] = zfit; out[6] = kslam::arrow_zg(zfit); out[7] = ac.Tn; out[8] = nK;
  return DRLGX_OK;
}

int drlgx_debug_inc_form(int P, int L0, int n_re, int pc, int P_max, int L_max, int LG, int lds_bytes, int32_t out[DRLGX_INC_FORM_N]) {
  if (!out || P < 2 || P > P_max || P_max > 65535 || L0 < 0 || L0 > L_max || L_max > 32767 || n_re < 0 || n_re > L0 || n_re > kslam::IncCarve::INF ||
      pc < 1 || pc > P_max || LG < 1 || LG > (1 << 20) || lds_bytes < 0 || lds_bytes > kslam::kLdsBudget)
    return DRLGX_E_INVALID;
  for (int i = 0; i < DRLGX_INC_FORM_N; ++i) out[i] = 0;
  // (as inc_plan: the simulator's region of the fused step at the launch's pose bound; the decisions do not depend on where the
  // calling kernel's own carve begins, so the stage kernels' offset 0 stands for all of them)
  const kslam::IncCarve c(P, L0, L_max, drlgx_sim_lds_bytes(LG, pc), (size_t)lds_bytes, 0);
  out[0] = c.feasible;
  if (!c.feasible) return DRLGX_OK;
  out[1] = c.lds_panel; out[2] = c.wide; out[3] = c.snt;
  const bool streamed = kslam::inc_streams(c.snt, c.wide, n_re, c.n1, c.a0);
  out[4] = streamed;
  int nw = 0;
  for (int b0 = 0; b0 < n_re; ++nw) {  // (inc_post's two loops)
    const int left = n_re - b0;
    const int nt = streamed ? kslam::inc_stream_tiles(c.snt, left) : kslam::inc_batch_wide(c.wide, left) ? 2 : 1;
    out[6 + nw] = nt;
    b0 += 8 * nt < left ? 8 * nt : left;
  }
  out[5] = nw;
  return DRLGX_OK;
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
  else if (arrow_ntw(S.L_max) == 0)
    hipLaunchKernelGGL((kslam::k_slam_arrow<0>), grid, block, kslam::kLdsBudget, st, DRLGX_KS_ARG(S), sel, kslam::kLdsBudget);
  else
    hipLaunchKernelGGL((kslam::k_slam_arrow<kslam::kArrowRegTiles>), grid, block, kslam::kLdsBudget, st, DRLGX_KS_ARG(S), sel, kslam::kLdsBudget);
}
