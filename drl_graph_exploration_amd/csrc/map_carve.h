// LDS layout of the virtual-map stage (k_map.hip: map_body): the ONE place that says where each of its arrays lies and how
// many bytes they take together.  The kernel carves its pointers from it, the host sizes the launch from it, the fused step
// (k_step.hip) reads from it where the map stage's pose tables end and its cell masks begin, the simulator's region
// (drlgx_sim_lds_bytes) is made wide enough for the pose tables with it, and drlgx_create refuses a map it cannot hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define DRLGX_LO_TAB 16  // states of the occupancy ladder: 4 bits per next state in DrlgxState::lo_tocc / lo_tfree

namespace kmap {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = 64;         // candidate cells per pose: an 8 x 8 slot grid whatever the window width W <= 8
constexpr int kPairsPerPose = 40;  // in-range cells per pose the compact stage has room for (the disc of radius max_range
                                   // holds ~28 cell centres of the 7 x 7 window, never more than 32; the 8 x 8 window's disc
                                   // up to 41: the host keeps such a sensor on the resident form, DrlgxState::disc_cells)
constexpr size_t kLdsBudget = 160 * 1024;  // LDS of a CU: what one workgroup of the map kernel may take

// pc: poses the per-pose tables hold (the launch's pose bound); chunk: poses per A / C pass; V: cells;
// compact: the form of k_map_c (one mask per cell, the stage indexed through sidx).  All members: byte offsets.
struct MapCarve {
  static constexpr int kSp = 4, kSi = 6, kSl = 9;  // doubles per pose of the three pose tables
  // the pose tables come first: the fused step's SLAM stage writes sp / si in place, and they must end inside the region the
  // simulator wave has left by then
  __host__ __device__ static constexpr size_t pose_tables_bytes(int pc) { return (size_t)pc * (kSp + kSi + kSl) * sizeof(double); }

  size_t sp = 0;       // double [pc][4] x y c s
  size_t si = 0;       // double [pc][6] pose information
  size_t sl = 0;       // double [pc][9] its LLT factor + reciprocals of the diagonal
  size_t stage = 0;    // double [chunk][kSlots][3]; compact: [chunk * kPairsPerPose][3]
  size_t mask = 0;     // u64 [V] poses that update the cell
  size_t omask = 0;    // u64 [V] poses that see the cell; compact: the same array as mask
  size_t scratch = 0;  // double [kWaves]
  size_t lpv = 0;      // double [DRLGX_LO_TAB] ladder state -> cell probability
  size_t bbox = 0;     // int [pc][4] min_row max_row min_col max_col
  size_t worg = 0;     // int [pc][2] window origin row, col
  size_t pskip = 0;    // int [pc]
  size_t lmc = 0;      // int [V] estimated landmarks per cell
  size_t pcount = 0;   // int: number of (pose, cell) pairs in range
  size_t plist = 0;    // u16 [chunk * kSlots] their pair indices
  size_t sidx = 0;     // u16 [chunk][kSlots] compact: stage entry of (pose, window slot); absent otherwise
  size_t bytes = 0;    // all of it

  __host__ __device__ constexpr MapCarve(int pc, int chunk, int V, bool compact) {
    const size_t npc = (size_t)pc, nch = (size_t)chunk, nv = (size_t)V;
    si = sp + npc * kSp * sizeof(double);
    sl = si + npc * kSi * sizeof(double);
    stage = sl + npc * kSl * sizeof(double);
    mask = stage + nch * (compact ? kPairsPerPose : kSlots) * 3 * sizeof(double);
    omask = compact ? mask : mask + nv * sizeof(uint64_t);
    scratch = omask + nv * sizeof(uint64_t);
    lpv = scratch + kWaves * sizeof(double);
    bbox = lpv + DRLGX_LO_TAB * sizeof(double);
    worg = bbox + npc * 4 * sizeof(int);
    pskip = worg + npc * 2 * sizeof(int);
    lmc = pskip + npc * sizeof(int);
    pcount = lmc + nv * sizeof(int);
    plist = pcount + sizeof(int);
    sidx = plist + nch * kSlots * sizeof(uint16_t);
    bytes = (compact ? sidx + nch * kSlots * sizeof(uint16_t) : sidx) + 16;
  }
};
// anchors: the bench state (41 poses in one chunk, the 40 m map at resolution 1), both forms.  (108 456 and 77 288 bytes by the
// formulas this struct replaced; recomputed when the ladder's 256-byte transition table left the carve and its value table
// went from 64 to 16 states: 640 bytes less.)
static_assert(MapCarve(41, 41, 1600, false).bytes == 107816, "resident carve of the map stage moved");
static_assert(MapCarve(41, 41, 1600, true).bytes == 76648, "compact carve of the map stage moved");
static_assert(MapCarve(41, 41, 1600, false).stage == MapCarve::pose_tables_bytes(41), "the stage follows the pose tables");

}  // namespace kmap
