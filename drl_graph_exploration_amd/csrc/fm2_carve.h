// Memory layout of the FastMarginals2 update (k_fm2.hip: k_fm2_update): the ONE place that says how many predicted measurements a
// candidate may have, how large the LDS Gauss-Jordan buffer therefore is, and where each array of a candidate's HBM scratch lies.
// The kernel takes its pointers from it; the host (drlgx_engine.cpp) sizes the scratch from it.
// Plain C++ (constexpr functions are host and device functions to the HIP compiler): a host program can include it alone.
#pragma once
#include <stddef.h>

namespace kfm2 {

constexpr int kFm2MaxMeas = 256;  // predicted measurements of one candidate: T is [2 nm][2 nm]
constexpr int kT = 256;           // threads of every workgroup of k_fm2.hip
// LDS of spd_inverse on T: the pivot column, then the pivot row, 2 kFm2MaxMeas doubles each
constexpr int kGjHalf = 2 * kFm2MaxMeas, kGjDoubles = 2 * kGjHalf;
static_assert(kGjDoubles == 2 * 2 * kFm2MaxMeas && kGjDoubles * sizeof(double) == 8192, "a column and a row of T at the cap: 8 KiB at 256");

// Scratch of one candidate for plans of up to A_max actions and up to nm_max predicted measurements.
struct Fm2Scratch {
  static constexpr int kUWaves = kT / 64;  // waves that own a slab of U
  // doubles (offsets)
  size_t cov_new = 0;  // [A][9] covariance of new pose b after its odometry factor
  size_t F = 0;        // [A][9] F_b = -H1 H0
  size_t Fs = 0;       // [A][9] Fs_b = F_b ... F_0
  size_t NN = 0;       // [A][A][9] Sigma(new a, new b), a <= b
  size_t J = 0;        // [nm][10] whitened Jx (2x3), Jl (2x2) of every predicted measurement
  size_t T = 0;        // [2 nm][2 nm] I + A Sigma A^T, then its inverse
  size_t U = 0;        // [kUWaves][2 nm][3] A Sigma(., x_i) of the block a wave is reducing (landmarks: [2 nm][2])
  size_t u_slab = 0;   // doubles of one wave's slab of U
  size_t newp = 0;     // [A][4] predicted poses (x y cos sin)
  size_t total = 0;    // all of it, 64 doubles to spare
  // ints (offsets)
  size_t mk = 0;      // [nm] measurement -> new pose index
  size_t mj = 0;      // [nm] measurement -> landmark slot
  size_t itotal = 0;  // both

  constexpr __attribute__((always_inline)) Fm2Scratch(int A_max, int nm_max) {
    const size_t A = (size_t)A_max, nm = (size_t)nm_max;
    F = cov_new + 9 * A;
    Fs = F + 9 * A;
    NN = Fs + 9 * A;
    J = NN + 9 * A * A;
    T = J + 10 * nm;
    U = T + 4 * nm * nm;
    u_slab = 6 * nm;
    newp = U + kUWaves * u_slab;
    total = newp + 4 * A + 64;
    mj = mk + nm;
    itotal = mj + nm;
  }
};

// anchors: the scratch at the measurement cap and the plan lengths the project uses, by the formula this struct replaced
constexpr size_t fm2_scratch_formula(size_t A, size_t nm) { return 31 * A + 9 * A * A + 34 * nm + 4 * nm * nm + 64; }
static_assert(Fm2Scratch(32, 256).total == fm2_scratch_formula(32, 256), "default_config(40) (the default engine, bench.py's 40 m map) moved");
static_assert(Fm2Scratch(39, 256).total == fm2_scratch_formula(39, 256), "bench.py's config 5 (default_config(50): 39 actions) moved");
static_assert(Fm2Scratch(9, 256).total == fm2_scratch_formula(9, 256), "the worlds of tests/fm2_cases.py, tests/slam_og_cases.py moved");
static_assert(Fm2Scratch(128, 256).total == fm2_scratch_formula(128, 256), "the 128-action Dubins engine (scripts/micro/em_plan_dubins.py) moved");
static_assert(Fm2Scratch(32, 256).itotal == 2 * kFm2MaxMeas, "mk | mj at the measurement cap");

}  // namespace kfm2
