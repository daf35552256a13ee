// Dev tool (no GPU): csrc/arrow_carve.h against the layout formulas it replaced, over a grid of counts and capacities.
//   c++ -std=c++17 -O1 -fsanitize=address,undefined -I drl_graph_exploration_amd/csrc scripts/arrow_carve_sweep.cpp -o /tmp/arrow_carve_sweep && /tmp/arrow_carve_sweep
// Prints the number of cases and of differences (exit status 1 if any) and the totals that the header's static_asserts pin.
// `old_*`: the expressions of arrow_body's carve, arrow_small_bytes, arrow_lds_bytes and drlgx_slam_ws_doubles before the header.
#include <algorithm>
#include <cstdio>
#include "arrow_carve.h"

namespace old {
using std::max;
constexpr int kThreads = 512, kWaves = kThreads / 64, kLdsBudget = 160 * 1024, kFastTilesArrow = 8, kArrowRegTiles = 20, REC = 12;
constexpr int kSegLog = 3, kSeg = 1 << kSegLog;
size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }
size_t sweep_region_doubles(size_t N) {
  const size_t a = N * (N + 1) / 2 + 6 * N + 64, b = 64 * N + 1024;
  return a > b ? a : b;
}
size_t arrow_small_bytes(int P, int L, int M) {
  const size_t MW = (size_t)(P + 63) >> 6;
  return (size_t)P * (4 + 6 + 9 + 9 + 9) * 8 + (size_t)L * (2 + 8) * 8 + (((size_t)(P + 2) * 4 + 7) & ~(size_t)7) +
         (size_t)L * MW * 8 + 64;
}
size_t arrow_lds_bytes(int P_max, int L_max, int M_max) {
  const size_t N = 16 * (((size_t)2 * L_max + 1 + 15) / 16);
  const size_t Tn = N / 16;
  const size_t sys = N <= 16 * kFastTilesArrow ? sweep_region_doubles(N)
                     : Tn * (Tn + 1) / 2 <= (size_t)kArrowRegTiles * (kWaves - 1) ? 32 * N + 1280 : 1280;
  return arrow_small_bytes(P_max, L_max, M_max) + sys * 8 + 64;
}
size_t ws_doubles(int P_max, int L_max, int M_max) {
  const size_t ldx = (size_t)((2 * L_max + 1 + 3 + 3) & ~3);
  const size_t n = (size_t)3 * P_max * ldx + (size_t)24 * P_max + (size_t)(P_max / kSeg + 2) * 3 * ldx + (size_t)(2 * L_max + 17) * (2 * L_max + 17) + (size_t)32 * (2 * L_max + 17) +
                   (size_t)M_max * REC + ((size_t)L_max * P_max * 2 + 7) / 8 + 16;
  return (n + 31) & ~(size_t)31;
}
struct Ws { size_t X, Ti, Sl, Sr, sepR, rec_ws, Aws, pws, obs; };
Ws ws_chain(int P_max, int L_max, int M_max) {  // (S.P_max -> P_max ...; wsd counted from 0)
  Ws w;
  size_t wsd = 0;
  w.X = wsd; wsd += (size_t)3 * P_max * (size_t)((2 * L_max + 1 + 3 + 3) & ~3);
  w.Ti = wsd; wsd += (size_t)6 * P_max;
  w.Sl = wsd; wsd += (size_t)9 * P_max;
  w.Sr = wsd; wsd += (size_t)9 * P_max;
  w.sepR = wsd; wsd += (size_t)(P_max / kSeg + 2) * 3 * (size_t)((2 * L_max + 1 + 3 + 3) & ~3);
  w.rec_ws = wsd; wsd += (size_t)M_max * REC;
  w.Aws = wsd; wsd += (size_t)(2 * L_max + 17) * (2 * L_max + 17);
  w.pws = wsd; wsd += (size_t)32 * (2 * L_max + 17);
  w.obs = wsd;
  return w;
}
struct Carve {
  int np, ncol, Tn, N, ncx, ldx, MW, nsep;
  bool c_lds, c_reg, obs_lds, xs_lds, rec_lds;
  size_t thp, Dd, Al, GL, GR, thl, lamb, mstart, bad, lmask, obs, U, rec, u_free, off;
};
Carve carve(int P, int L, int M, int NTW, int lds_bytes, bool mk_panel) {  // (pointers counted from smem_raw = 0)
  Carve c;
  const int np = 2 * L, ncol = np + 1;
  const int Tn = (ncol + 15) / 16, N = 16 * Tn;
  const int ntiles = Tn * (Tn + 1) / 2;
  const bool c_lds = Tn <= kFastTilesArrow;
  const int ncx = mk_panel ? ncol + 3 : ncol;
  const int ldx = (ncol + 3 + 3) & ~3;
  const bool c_reg = !c_lds && NTW > 0 && ntiles <= NTW * (kWaves - 1);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t q = off;
    off += up8(bytes);
    return q;
  };
  c.thp = take((size_t)P * 4 * 8);
  c.Dd = take((size_t)P * 6 * 8);
  c.Al = take((size_t)P * 9 * 8);
  c.GL = take((size_t)P * 9 * 8);
  c.GR = take((size_t)P * 9 * 8);
  c.thl = take((size_t)L * 2 * 8);
  c.lamb = take((size_t)L * 8 * 8);
  c.mstart = take((size_t)(P + 2) * 4);
  c.bad = take(8);
  const int MW = (P + 63) >> 6;
  c.lmask = take((size_t)L * MW * 8);
  off = (off + 31) & ~(size_t)31;
  const size_t sys_bytes = (c_lds ? sweep_region_doubles(N) : c_reg ? (size_t)32 * N + 1280 : (size_t)1280) * 8;
  c.obs = 0;
  c.obs_lds = false;
  if (off + sys_bytes + up8((size_t)L * P * 2) + 32 <= (size_t)lds_bytes) {
    c.obs = off; off += (up8((size_t)L * P * 2) + 31) & ~(size_t)31;
    c.obs_lds = true;
  }
  const int nsep = (P + kSeg - 1) / kSeg;
  const size_t xs_bytes = (size_t)nsep * 3 * ldx * 8;
  c.U = off;
  const bool xs_lds = off + max(sys_bytes, xs_bytes) <= (size_t)lds_bytes;
  off += xs_lds ? max(sys_bytes, xs_bytes) : sys_bytes;
  size_t u_free = (size_t)(off - c.U);
  c.rec = 0;
  c.rec_lds = false;
  if (off + (size_t)M * REC * 8 <= (size_t)lds_bytes) {
    c.rec = off; off += (size_t)M * REC * 8;
    c.rec_lds = true;
  } else {
    u_free = (size_t)lds_bytes - c.U;
  }
  c.np = np; c.ncol = ncol; c.Tn = Tn; c.N = N; c.ncx = ncx; c.ldx = ldx; c.MW = MW; c.nsep = nsep;
  c.c_lds = c_lds; c.c_reg = c_reg; c.xs_lds = xs_lds; c.u_free = u_free; c.off = off;
  return c;
}
}  // namespace old

static long long cases = 0, diffs = 0;
#define CMP(a, b)                                                                     \
  do {                                                                                \
    if ((size_t)(a) != (size_t)(b)) {                                                 \
      if (diffs++ < 20) std::printf("DIFF %s: %zu != %zu  (%s)\n", #a, (size_t)(a), (size_t)(b), what); \
    }                                                                                 \
  } while (0)

static void one_carve(int P, int L, int M, int NTW, int lds, bool mk) {
  char what[96];
  std::snprintf(what, sizeof what, "P %d L %d M %d NTW %d lds %d mk %d", P, L, M, NTW, lds, (int)mk);
  const old::Carve o = old::carve(P, L, M, NTW, lds, mk);
  const kslam::ArrowCarve n(P, L, M, NTW, lds, mk);
  ++cases;
  CMP(n.np, o.np); CMP(n.ncol, o.ncol); CMP(n.ncx, o.ncx); CMP(n.ldx, o.ldx); CMP(n.Tn, o.Tn); CMP(n.N, o.N); CMP(n.MW, o.MW); CMP(n.nsep, o.nsep);
  CMP(n.c_lds, o.c_lds); CMP(n.c_reg, o.c_reg); CMP(n.obs_lds, o.obs_lds); CMP(n.xs_lds, o.xs_lds); CMP(n.rec_lds, o.rec_lds);
  CMP(n.thp, o.thp); CMP(n.Dd, o.Dd); CMP(n.Al, o.Al); CMP(n.GL, o.GL); CMP(n.GR, o.GR); CMP(n.thl, o.thl); CMP(n.lamb, o.lamb);
  CMP(n.mstart, o.mstart); CMP(n.bad, o.bad); CMP(n.lmask, o.lmask); CMP(n.U, o.U); CMP(n.u_free, o.u_free); CMP(n.end, o.off);
  if (o.obs_lds) CMP(n.obs, o.obs);
  if (o.rec_lds) CMP(n.rec, o.rec);
  CMP(kslam::arrow_ldx(L), o.ldx);
  if (o.c_lds) CMP(kslam::arrow_packed_doubles((size_t)o.N), old::sweep_region_doubles((size_t)o.N));
}
static void one_cap(int P_max, int L_max, int M_max) {
  char what[96];
  std::snprintf(what, sizeof what, "P_max %d L_max %d M_max %d", P_max, L_max, M_max);
  const old::Ws o = old::ws_chain(P_max, L_max, M_max);
  const kslam::ArrowWs n(P_max, L_max, M_max);
  ++cases;
  CMP(n.X, o.X); CMP(n.Ti, o.Ti); CMP(n.Sl, o.Sl); CMP(n.Sr, o.Sr); CMP(n.sepR, o.sepR); CMP(n.rec, o.rec_ws); CMP(n.A, o.Aws); CMP(n.pws, o.pws); CMP(n.obs, o.obs);
  CMP(n.total, old::ws_doubles(P_max, L_max, M_max));
  CMP(kslam::ArrowCarve::min_bytes(P_max, L_max), old::arrow_lds_bytes(P_max, L_max, M_max));
  CMP(kslam::ArrowCarve::tables_bytes(P_max, L_max) + 56, old::arrow_small_bytes(P_max, L_max, M_max));
}

int main() {
  // every P in 1..256 and L in 0..500 (so: P = 1, multiples of 8 plus 0 or 1, L = 0, 6, 7, 63, 64, 127, 128)
  for (int P = 1; P <= 256; ++P)
    for (int L = 0; L <= 500; ++L) {
      const int Ms[] = {0, 1, P, 12 * P + 20, 30 * P, 45 * P};
      const size_t need = old::arrow_lds_bytes(P, L, 0);
      // the whole LDS, what the host admits a capacity by, and a request that the tables alone overrun
      const int ldss[] = {old::kLdsBudget, (int)std::min<size_t>(need, old::kLdsBudget), 64 * 1024};
      for (int M : Ms)
        for (int lds : ldss)
          for (int NTW : {0, old::kArrowRegTiles})
            for (int mk = 0; mk < 2; ++mk) one_carve(P, L, M, NTW, lds, mk != 0);
      // capacities at and above the counts
      for (int dP : {0, 1, 7})
        for (int dL : {0, 1, 27})
          for (int M : Ms) one_cap(P + dP, L + dL, M + dP);
    }
  std::printf("ws / lds-min  config 5 (127, 127, 3800): %zu %zu\n", old::ws_doubles(127, 127, 3800), old::arrow_lds_bytes(127, 127, 3800));
  std::printf("ws / lds-min  500 landmarks (80, 500, 3600): %zu %zu\n", old::ws_doubles(80, 500, 3600), old::arrow_lds_bytes(80, 500, 3600));
  std::printf("ws / lds-min  default engine (41, 100, 512): %zu %zu\n", old::ws_doubles(41, 100, 512), old::arrow_lds_bytes(41, 100, 512));
  std::printf("%lld cases, %lld differences\n", cases, diffs);
  return diffs ? 1 : 0;
}
