// LDS layout of the dense solver (k_slam.hip: SlamCtx): the ONE place that says where each of its arrays lies in the dynamic
// LDS, what is parked in the slack of the sweep region, and how many bytes a solve or an engine needs.  SlamCtx::setup takes its
// pointers from it, slam_finish and k_step choose the records' placement by it, the host (drlgx_slam_in_lds,
// drlgx_step_fusable) admits capacities by it.
// Plain C++ (constexpr functions are host and device functions to the HIP compiler): a host program can include it alone.
#pragma once
#include <stddef.h>
#include "arrow_carve.h"

namespace kslam {

#define SLAM_CARVE_FN constexpr __attribute__((always_inline))  // (also inside the kernels: no call)
// The landmark-first dense solve (k_slam.hip) serves systems of up to kDenseTiles tile rows (N = 160: 53 poses).  Up to
// kFastTiles the sweep gives every wave ONE tile row; with nine and ten rows (43 .. 53 poses) two light rows share a wave
// (sweep_packed_fast).  That keeps such updates off the pose-chain solver (k_slam_arrow.hip: ~230 us at 46 poses against
// ~65 us for the dense solve at 41).
constexpr int kFastTiles = 8;  // N = 128: <= 42 poses
constexpr int kDenseTiles = 10;

// rows of the padded system of P poses: 3 P pivots + the rhs row, in 16 x 16 MFMA tiles
SLAM_CARVE_FN size_t slam_dim(int P) { return 16 * (((size_t)3 * P + 1 + 15) / 16); }
// The sweep region: the packed triangle or the panels of sweep_packed_fast that alias it (arrow_packed_doubles is
// sweep_region_doubles of k_sweep.hip; k_slam.hip asserts it up to 16 kDenseTiles).  Two sizes of it are in use:
//   slam_sys_doubles   what a solve of N rows carves.  The sweep addresses its panels with stride 16 N (SwL{A, 16 N}: 64 N + 1024
//                      doubles), loads and stores the triangle up to row N, and its idle tile rows (sweep_role<-1>) publish
//                      nothing: the region at the solve's own N is all that sweep_packed_fast<FT> touches, whatever FT.
//   slam_host_doubles  what the host admits a capacity by: the region at max(N, 16 kFastTiles).  Nothing in the kernels needs the
//                      larger value - up to 37 poses (N < 128) the host sets 10 .. 55 KB aside that no solve carves.  It only
//                      ever refuses more, and both values are kept as they were.
SLAM_CARVE_FN size_t slam_sys_doubles(size_t N) { return arrow_packed_doubles(N); }
SLAM_CARVE_FN size_t slam_host_doubles(size_t N) { return arrow_packed_doubles(N > 16 * (size_t)kFastTiles ? N : 16 * (size_t)kFastTiles); }

// LDS of one solve of P poses with room for Lb landmarks and Mb factors, carved from byte `base` of the dynamic LDS.  All
// offsets in bytes from the start of the dynamic LDS; every small array is rounded up to 8 bytes.
struct SlamCarve {
  static constexpr int kRec = ArrowWs::kRec;  // doubles per factor record (REC, k_slam_common.hip)
  static constexpr int kPark = 9;             // doubles per pose of a parked table: block (6, lower triangle) + gradient (3)
  static SLAM_CARVE_FN size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }
  // doubles from `sys` to the two parked tables (below) of a system of N rows and P poses
  static SLAM_CARVE_FN size_t park_c2_doubles(size_t N) { return N * (N + 1) / 2; }
  static SLAM_CARVE_FN size_t park_own_doubles(size_t N, size_t P) { return park_c2_doubles(N) + kPark * P; }

  int np = 0, Tn = 0, N = 0, MW = 0;  // pivots; tile rows, N = 16 Tn; mask words per landmark
  size_t thp = 0;     // double [P][4] theta of the poses (x, y, cos, sin)
  size_t odl = 0;     // double [P][4] measured odometry between pose i and i + 1
  size_t thl = 0;     // double [Lb][2] theta of the landmarks
  size_t lamb = 0;    // double [Lb][8] Lambda_jj (3), its inverse (3), eta_j (2)
  size_t mstart = 0;  // int [P + 2] first factor of each pose
  size_t lstart = 0;  // int [Lb + 2] first entry of each landmark's factor list
  size_t pstart = 0;  // int [Lb + 2] first work item (pair of list entries) of each landmark
  size_t mp = 0;      // u16 [Mb] pose of the factor
  size_t ml = 0;      // u16 [Mb] landmark of the factor
  size_t lfac = 0;    // u16 [Mb] the per-landmark factor lists
  size_t pairlm = 0;  // u16 [Mb / 2 + Lb + 2] landmark of each work item of the landmark marginals
  size_t bad = 0;     // int [2]: numeric flag, pair / work counter (SlamCtx::numeric_flag, pair_count, work_counter)
  size_t lmask = 0;   // u64 [Lb][MW] poses that observe the landmark
  size_t sys = 0;     // double [slam_sys_doubles(N)] the sweep region, 32-byte aligned: packed triangle, then the sweep's panels
  // Parked behind the packed triangle, inside the sweep region, while the front end assembles the pose blocks: the second-key /
  // prior contributions (slot 0: the prior) and the eight-lane own-factor sums, kPark doubles per pose each.  The region holds
  // at least 6 N + 64 doubles behind the triangle and 2 kPark P = 18 P <= 6 (N - 1) because 3 P + 1 <= N (parks_fit below); they
  // are dead before the sweep turns the region into its panels.
  size_t park_c2 = 0, park_own = 0;
  size_t rec = 0;     // double [Mb][kRec] factor records, when they are in LDS (else: the workspace, ArrowWs::rec)
  size_t obs = 0;     // u16 [Lb][P] factor index + 1 of (landmark, pose), behind the records
  size_t small = 0;         // bytes of the small arrays, 32 of them for the alignment of `sys`
  size_t with_records = 0;  // upper end of the carve with records and observation table in LDS (from 0: includes `base`)

  SLAM_CARVE_FN SlamCarve(int P, int Lb, int Mb, size_t base = 0) {
    np = 3 * P;
    Tn = (np + 1 + 15) / 16; N = 16 * Tn;  // (= slam_dim(P), in the kernels' int arithmetic)
    MW = (P + 63) >> 6;
    const size_t nP = (size_t)P, nL = (size_t)Lb, nM = (size_t)Mb;
    thp = base;
    odl = thp + up8(nP * 4 * 8);
    thl = odl + up8(nP * 4 * 8);
    lamb = thl + up8(nL * 2 * 8);
    mstart = lamb + up8(nL * 8 * 8);
    lstart = mstart + up8((nP + 2) * 4);
    pstart = lstart + up8((nL + 2) * 4);
    mp = pstart + up8((nL + 2) * 4);
    ml = mp + up8(nM * 2);
    lfac = ml + up8(nM * 2);
    pairlm = lfac + up8(nM * 2);
    bad = pairlm + up8((nM / 2 + nL + 2) * 2);
    lmask = bad + 8;
    const size_t end_small = lmask + up8(nL * MW * 8);
    sys = arrow_up(end_small, 32);
    park_c2 = sys + park_c2_doubles((size_t)N) * 8;
    park_own = sys + park_own_doubles((size_t)N, nP) * 8;
    rec = sys + slam_sys_doubles((size_t)N) * 8;
    obs = rec + nM * kRec * 8;
    small = end_small - base + 32;
    with_records = base + small + slam_sys_doubles((size_t)N) * 8 + nM * kRec * 8 + up8(nL * nP * 2);
  }
  // LDS the dense solver cannot do without at capacity: the small arrays and the sweep region at the host's size (records and
  // observation table overflow to the workspace).  The fused step adds the simulator's region in front.
  static SLAM_CARVE_FN size_t min_bytes(int P_max, int L_max, int M_max) {
    return SlamCarve(P_max, L_max, M_max).small + slam_host_doubles(slam_dim(P_max)) * 8;
  }
  // the dense solver serves capacities up to kDenseTiles tile rows whose min_bytes fit behind `front` bytes of someone else's
  static SLAM_CARVE_FN bool fits(int P_max, int L_max, int M_max, size_t front, size_t budget) {
    return slam_dim(P_max) <= 16 * (size_t)kDenseTiles && front + min_bytes(P_max, L_max, M_max) <= budget;
  }
};

constexpr bool slam_parks_fit() {
  for (int P = 1; 3 * P + 1 <= 16 * kDenseTiles; ++P) {
    const SlamCarve c(P, 0, 0);
    if (c.park_own + SlamCarve::kPark * (size_t)P * 8 > c.rec) return false;
  }
  return true;
}
static_assert(slam_parks_fit(), "the parked tables must lie inside the sweep region for every N <= 16 kDenseTiles");
// anchors: small, with_records (from base 0) and min_bytes at capacities the project uses, by the device formulas this struct replaced
static_assert(SlamCarve(41, 8, 492).small == 7088 && SlamCarve(41, 8, 492).with_records == 128704 && SlamCarve::min_bytes(41, 8, 492) == 80816,
              "the default engine (41 poses, 40 m map) moved");
static_assert(SlamCarve(41, 100, 512).small == 16248 && SlamCarve(41, 100, 512).with_records == 147328 && SlamCarve::min_bytes(41, 100, 512) == 89976,
              "bench.py's 41-pose engine moved");
static_assert(SlamCarve(53, 100, 756).small == 18768 && SlamCarve(53, 100, 756).with_records == 213176 && SlamCarve::min_bytes(53, 100, 756) == 130000,
              "53 poses at the capacities of the pose sweep (scripts/bench_vs_poses.py 54) moved");
static_assert(slam_dim(53) == 16 * kDenseTiles && slam_dim(42) == 16 * kFastTiles, "the pose counts the comments name");

#undef SLAM_CARVE_FN
}  // namespace kslam
