// Dev tool (no GPU): csrc/slam_carve.h against the three layout formulas of the dense solver that it replaced.
//   c++ -std=c++17 -O2 -fsanitize=address,undefined -I drl_graph_exploration_amd/csrc scripts/slam_carve_sweep.cpp -o /tmp/slam_carve_sweep && /tmp/slam_carve_sweep
// Over P 1..53, L 0..600, M 0..6000 and three carve bases (0 and the simulator's region at two pose bounds) it compares
//   - every offset, `small` and `with_records` with SlamCtx::setup / small_bytes / big_fits as they were (any difference: exit 1),
//   - the host predicates drlgx_slam_in_lds and the SLAM terms of drlgx_step_fusable, old (slam_small_bytes: no rounding, M * 7,
//     + 224) and new (SlamCarve::fits).  The new ones are exact, so they admit what the old ones refused by 145..180 bytes of
//     accidental slack: such flips are counted; a flip the other way, or a new predicate that is true where the device's own total
//     exceeds the budget, is an error (exit 1).
// Then the table of the capacities that the tests, bench.py and scripts/bench_*.py create engines with, at every pose bound the
// engine may pass: old and new decisions and the number that flip (expected: none).
#include <algorithm>
#include <cstdio>
#include "slam_carve.h"

namespace old {
constexpr int kLdsBudget = 160 * 1024, kFastTiles = 8, kDenseTiles = 10, REC = 12, DRLGX_MT_STRIDE = 626;
size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }
size_t sweep_region_doubles(size_t N) {
  const size_t a = N * (N + 1) / 2 + 6 * N + 64, b = 64 * N + 1024;
  return a > b ? a : b;
}
// ---- device: SlamCtx::small_bytes, big_fits, setup ----
size_t small_bytes(int P, int Lb, int Mb) {
  const size_t MW = (size_t)(P + 63) >> 6;
  return up8((size_t)P * 32) * 2 + up8((size_t)Lb * 16) + up8((size_t)Lb * 64) + up8((size_t)(P + 2) * 4) + up8((size_t)(Lb + 2) * 4) * 2 +
         up8((size_t)Mb * 2) * 3 + up8((size_t)(Mb / 2 + Lb + 2) * 2) + 8 + up8((size_t)Lb * MW * 8) + 32;
}
size_t big_total(size_t off, int P, int Lb, int Mb) {  // (big_fits: this <= lds_bytes)
  const size_t N = 16 * (((size_t)3 * P + 1 + 15) / 16);
  return off + small_bytes(P, Lb, Mb) + sweep_region_doubles(N) * 8 + (size_t)Mb * REC * 8 + up8((size_t)Lb * P * 2);
}
struct Carve {
  int np, Tn, N, MW;
  size_t thp, odl, thl, lamb, mstart, lstart, pstart, mp, ml, lfac, pairlm, bad, lmask, A, c2buf, ownsum, rec, obs, end;
};
Carve setup(size_t off, int P, int Lb, int Mb) {  // (pointers counted from smem_raw = 0; kBigLds)
  Carve c;
  c.np = 3 * P;
  c.Tn = (c.np + 1 + 15) / 16; c.N = 16 * c.Tn;
  c.MW = (P + 63) >> 6;
  auto take = [&](size_t bytes) { size_t q = off; off += up8(bytes); return q; };
  c.thp = take((size_t)P * 4 * 8);
  c.odl = take((size_t)P * 4 * 8);
  c.thl = take((size_t)Lb * 2 * 8);
  c.lamb = take((size_t)Lb * 8 * 8);
  c.mstart = take((size_t)(P + 2) * 4);
  c.lstart = take((size_t)(Lb + 2) * 4);
  c.pstart = take((size_t)(Lb + 2) * 4);
  c.mp = take((size_t)Mb * 2);
  c.ml = take((size_t)Mb * 2);
  c.lfac = take((size_t)Mb * 2);
  c.pairlm = take((size_t)(Mb / 2 + Lb + 2) * 2);
  c.bad = take(8);
  c.lmask = take((size_t)Lb * c.MW * 8);
  off = (off + 31) & ~(size_t)31;
  c.A = off; off += sweep_region_doubles(c.N) * 8;
  c.rec = off; off += (size_t)Mb * REC * 8;
  c.obs = off;
  c.end = off + up8((size_t)Lb * P * 2);
  c.c2buf = c.A + (size_t)c.N * (c.N + 1) / 2 * 8;  // (front: A + N (N + 1) / 2, ownsum = c2buf + 9 P)
  c.ownsum = c.c2buf + (size_t)9 * P * 8;
  return c;
}
// ---- host: k_slam_host.hip, k_step.hip ----
size_t slam_dim(int P_max) { return 16 * (((size_t)3 * P_max + 1 + 15) / 16); }
size_t slam_small_bytes(int P_max, int L_max, int M_max) {
  return (size_t)P_max * 64 + (size_t)L_max * 16 + (size_t)L_max * 64 + (size_t)L_max * 8 * ((P_max + 63) / 64) +
         (size_t)(P_max + 2) * 4 + (size_t)(L_max + 2) * 8 + (size_t)M_max * 7 + (size_t)L_max * 2 + 224;
}
bool slam_in_lds(int P_max, int L_max, int M_max) {
  const size_t n = slam_dim(P_max), nf = std::max<size_t>(n, 16 * kFastTiles);
  return n <= (size_t)16 * kDenseTiles && slam_small_bytes(P_max, L_max, M_max) + sweep_region_doubles(nf) * 8 <= (size_t)kLdsBudget;
}
bool step_fusable_slam(size_t sim_bytes, int Pb, int L_max, int M_max) {  // (drlgx_step_fusable without its map-stage term)
  const size_t nf = std::max<size_t>(slam_dim(Pb), 16 * kFastTiles);
  return slam_in_lds(Pb, L_max, M_max) && sim_bytes + slam_small_bytes(Pb, L_max, M_max) + sweep_region_doubles(nf) * 8 <= (size_t)kLdsBudget;
}
// drlgx_sim_lds_bytes (drlgx_dev.h; the map stage's pose tables: 19 doubles per pose, map_carve.h) - unchanged, restated because
// those headers need the HIP runtime
size_t sim_lds_bytes(int LG, int P_max) {
  size_t b = (size_t)2 * DRLGX_MT_STRIDE * 4 + (size_t)(2 * LG + 2) * 8 + (size_t)LG * 4 + 16;
  b = ((b + 7) & ~(size_t)7) + (size_t)2 * LG * 8;
  const size_t pt = (size_t)P_max * 19 * 8 + 32;
  if (P_max <= 64) b = b > pt ? b : pt;
  return (b + 31) & ~(size_t)31;
}
}  // namespace old

namespace nw {
constexpr size_t kLdsBudget = 160 * 1024;
bool slam_in_lds(int P_max, int L_max, int M_max) { return kslam::SlamCarve::fits(P_max, L_max, M_max, 0, kLdsBudget); }
bool step_fusable_slam(size_t sim_bytes, int Pb, int L_max, int M_max) { return kslam::SlamCarve::fits(Pb, L_max, M_max, sim_bytes, kLdsBudget); }
}  // namespace nw

static long long cases = 0, diffs = 0, errors = 0;
#define CMP(a, b)                                                                                         \
  do {                                                                                                    \
    if ((size_t)(a) != (size_t)(b)) {                                                                     \
      if (diffs++ < 20) std::printf("DIFF %s: %zu != %zu  (P %d L %d M %d base %d)\n", #a, (size_t)(a), (size_t)(b), what[0], what[1], what[2], what[3]); \
    }                                                                                                     \
  } while (0)

struct Flips {
  long long n = 0, admitted = 0, refused = 0, beyond = 0, old_true = 0, new_true = 0;
  void add(bool o, bool n_, size_t device_total, const char *name, int P, int L, int M, size_t base) {
    ++n;
    old_true += o; new_true += n_;
    if (!o && n_) ++admitted;
    if (o && !n_) {
      if (refused++ < 5) std::printf("ERROR %s: admitted -> refused at P %d L %d M %d base %zu\n", name, P, L, M, base);
    }
    if (n_ && device_total > nw::kLdsBudget) {
      if (beyond++ < 5) std::printf("ERROR %s: true beyond the budget (%zu) at P %d L %d M %d base %zu\n", name, device_total, P, L, M, base);
    }
  }
  void report(const char *name) {
    std::printf("%-34s %lld triples: old true %lld, new true %lld; refused -> admitted %lld, admitted -> refused %lld, true beyond the budget %lld\n",
                name, n, old_true, new_true, admitted, refused, beyond);
    errors += refused + beyond;
  }
};

static void one(int P, int L, int M, size_t base) {
  const kslam::SlamCarve n(P, L, M, base);
  ++cases;
  const int what[4] = {P, L, M, (int)base};
  const old::Carve o = old::setup(base, P, L, M);
  CMP(n.np, o.np); CMP(n.Tn, o.Tn); CMP(n.N, o.N); CMP(n.MW, o.MW);
  CMP(n.thp, o.thp); CMP(n.odl, o.odl); CMP(n.thl, o.thl); CMP(n.lamb, o.lamb); CMP(n.mstart, o.mstart); CMP(n.lstart, o.lstart);
  CMP(n.pstart, o.pstart); CMP(n.mp, o.mp); CMP(n.ml, o.ml); CMP(n.lfac, o.lfac); CMP(n.pairlm, o.pairlm); CMP(n.bad, o.bad);
  CMP(n.lmask, o.lmask); CMP(n.sys, o.A); CMP(n.park_c2, o.c2buf); CMP(n.park_own, o.ownsum); CMP(n.rec, o.rec); CMP(n.obs, o.obs);
  CMP(n.small, old::small_bytes(P, L, M));
  CMP(n.with_records, old::big_total(base, P, L, M));
  CMP(kslam::slam_sys_doubles((size_t)o.N), old::sweep_region_doubles((size_t)o.N));
  if (o.end > n.with_records && diffs++ < 20) std::printf("DIFF the carve ends beyond with_records (P %d L %d M %d)\n", P, L, M);
}

struct Config { const char *who; int P_max, L_max, M_max, LG; };
// default_config: L_max = min(num_landmarks, 127) unless given, M_max = max(64, 12 P_max) unless given, LG = num_landmarks
static const Config kConfigs[] = {
    {"default engine, tests (40 m map)", 41, 8, 492, 8},
    {"bench.py headline / lazy restore", 41, 100, 512, 100},
    {"bench.py look-ahead, 64 poses", 64, 100, 788, 100},
    {"bench.py default capacity 256", 256, 100, 3092, 100},
    {"bench.py / scripts config 5", 127, 127, 3800, 500},
    {"tests: 60 poses", 60, 8, 720, 8},
    {"tests: 64 poses, 60 landmarks", 64, 60, 768, 60},
    {"tests: 60 / 100 / 30 landmarks, 41", 41, 60, 492, 60},
    {"tests: 100 landmarks, 41 poses", 41, 100, 492, 100},
    {"tests: 20 m map, 30 landmarks", 41, 30, 492, 30},
    {"tests: 43 poses", 43, 8, 516, 8},
    {"tests: 86 poses", 86, 8, 1032, 8},
    {"tests: 90 poses", 90, 8, 1080, 8},
    {"tests: 127 poses", 127, 8, 1524, 8},
    {"tests: 200 poses", 200, 8, 2400, 8},
    {"tests: 256 poses (vecenv default)", 256, 8, 3072, 8},
    {"tests: 40 / 80 poses (vecenv)", 80, 8, 960, 8},
    {"tests: 500 landmarks, 80 poses", 80, 500, 3600, 500},
    {"tests: 500 landmarks, cap 127, 120", 120, 127, 3600, 500},
    {"tests: 200 poses, 500 landmarks", 200, 500, 3600, 500},
    {"tests: inc 100 lm, 64 poses", 64, 100, 768, 100},
    {"tests: inc 300 lm, 72 poses", 72, 127, 3240, 300},
    {"bench_vs_poses 54, 100 landmarks", 54, 100, 756, 100},
    {"bench_vs_poses 206, 100 landmarks", 206, 100, 2884, 100},
    {"bench_vs_poses 54, 8 landmarks", 54, 8, 756, 8},
    {"phase_profile_relin PP_CAP 50", 50, 100, 620, 100},
    {"phase_profile_relin PP_CAP 40", 40, 100, 500, 100},
    {"phase_profile_cap 100 lm, cap 53", 53, 100, 742, 100},
    {"determinism_check cap 53, 128 lm", 53, 128, 1590, 300},
    {"bit comparison (b): 54, 40 lm", 54, 40, 648, 40},
};

int main() {
  const size_t bases[3] = {0, old::sim_lds_bytes(100, 41), old::sim_lds_bytes(8, 53)};
  std::printf("carve bases: 0, %zu (simulator's region, 100 landmarks in the world, 41 poses), %zu (8 landmarks, 53 poses)\n", bases[1], bases[2]);
  Flips in_lds, fus[3];
  for (int P = 1; P <= 53; ++P) {
    for (int L = 0; L <= 600; ++L)
      for (int M = 0; M <= 6000; ++M) {
        for (size_t base : bases) one(P, L, M, base);
        const size_t dev = kslam::SlamCarve(P, L, M).small + kslam::slam_sys_doubles(kslam::slam_dim(P)) * 8;  // without records
        in_lds.add(old::slam_in_lds(P, L, M), nw::slam_in_lds(P, L, M), dev, "drlgx_slam_in_lds", P, L, M, 0);
        for (int b = 0; b < 3; ++b)
          fus[b].add(old::step_fusable_slam(bases[b], P, L, M), nw::step_fusable_slam(bases[b], P, L, M), bases[b] + dev, "drlgx_step_fusable", P, L, M, bases[b]);
      }
  }
  std::printf("%lld carves compared, %lld differences\n", cases, diffs);
  in_lds.report("drlgx_slam_in_lds");
  fus[0].report("drlgx_step_fusable (SLAM), base 0");
  fus[1].report("drlgx_step_fusable (SLAM), base 1");
  fus[2].report("drlgx_step_fusable (SLAM), base 2");
  // beyond the dense solver's reach both refuse
  for (int P = 54; P <= 300; ++P)
    if (old::slam_in_lds(P, 8, 64) || nw::slam_in_lds(P, 8, 64)) { std::printf("ERROR: %d poses admitted\n", P); ++errors; }

  std::printf("\nengine configurations of the repository, every pose bound Pb = 1 .. P_max (in_lds / fusable: bounds admitted, old -> new)\n");
  long long cfg_flips = 0;
  for (const Config &c : kConfigs) {
    int o_in = 0, n_in = 0, o_fu = 0, n_fu = 0, flips = 0;
    for (int Pb = 1; Pb <= c.P_max; ++Pb) {
      const size_t sim = old::sim_lds_bytes(c.LG, Pb);
      const bool a = old::slam_in_lds(Pb, c.L_max, c.M_max), b = nw::slam_in_lds(Pb, c.L_max, c.M_max);
      const bool f = old::step_fusable_slam(sim, Pb, c.L_max, c.M_max), g = nw::step_fusable_slam(sim, Pb, c.L_max, c.M_max);
      o_in += a; n_in += b; o_fu += f; n_fu += g;
      flips += (a != b) + (f != g);
    }
    const int Pd = std::min(c.P_max, 53);
    std::printf("  %-36s (%3d, %3d, %4d) LG %3d: in_lds %2d -> %2d, fusable %2d -> %2d, flips %d; min_bytes at %d poses %zu, sim %zu\n", c.who, c.P_max,
                c.L_max, c.M_max, c.LG, o_in, n_in, o_fu, n_fu, flips, Pd, kslam::SlamCarve::min_bytes(Pd, c.L_max, c.M_max), old::sim_lds_bytes(c.LG, Pd));
    cfg_flips += flips;
  }
  std::printf("flips among the repository's configurations: %lld\n", cfg_flips);
  std::printf("\nanchors: small / with_records / min_bytes\n");
  for (const Config &c : {kConfigs[0], kConfigs[1], Config{"53 poses at bench capacities", 53, 100, 756, 100}}) {
    const kslam::SlamCarve k(c.P_max, c.L_max, c.M_max);
    std::printf("  (%d, %d, %d): %zu %zu %zu\n", c.P_max, c.L_max, c.M_max, k.small, k.with_records, kslam::SlamCarve::min_bytes(c.P_max, c.L_max, c.M_max));
  }
  return (diffs || errors) ? 1 : 0;
}
