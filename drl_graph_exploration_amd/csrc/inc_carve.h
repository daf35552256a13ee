// LDS plan of the incremental (rank-k) belief update (k_inc.hip: inc_plan, inc_post) as plain C++: where each of its arrays lies in
// the dynamic LDS, whether an update fits at all, whether the covariance panel is staged in LDS or updated in place in HBM / L2,
// whether the second half of Y fits (wide batches), how many factor tiles a walk of the streamed form takes, and which of the forms
// serves an update of n_re re-observed landmarks.  The host's drlgx_debug_inc_form (k_slam_host.hip) answers from it.
// inc_plan / inc_post keep their own spelling of this arithmetic: taking it from here changed the register allocation of the fused
// step kernels ("Which form serves which case"), and their code object is held fixed.  k_inc.hip ties its constants to
// the ones below by static_assert, and tests/test_gpu_inc_forms.py holds the two spellings against each other through the paths
// the device takes (inc_stats) at every form.
// (constexpr functions are host and device functions to the HIP compiler: a host program can include it alone.)
#pragma once
#include <stddef.h>
#include "slam_carve.h"

namespace kslam {

#define INC_CARVE_FN constexpr __attribute__((always_inline))

// The carve of the update that brings an instance to P poses, from what is known BEFORE the step: L0, the landmark count of the
// previous update (the panel's), plus room for up to INEW landmarks seen for the first time.
//   sim_lds    drlgx_sim_lds_bytes(LG, pc): the simulator's region of the fused step at the launch's pose bound pc
//   lds_bytes  the dynamic LDS of the launch
//   smem_off   where the calling kernel's carve begins (the fused step: behind the simulator's region; the stage kernels: 0)
// All offsets in bytes from the start of the dynamic LDS.  The DECISIONS are taken for the same offset in every kernel (plan_off:
// the fused step's), so that the fused kernel and the stage kernels always run the same instantiation.
struct IncCarve {
  // (k_inc.hip: IYS, INF, INEW, kStreamKB, ISNT)
  static constexpr int IYS = 18;  // row stride (doubles) of the Y / U' / W' images: 16 columns in ks16 order + 2 pad (144 B)
  static constexpr int INF = 64;  // most bearing-range factors one step may add on this path
  static constexpr int INEW = 12;  // most landmarks one step may see for the first time on this path
  static constexpr int kStreamKB = 512;  // a Y image (n1 x a0 doubles) beyond this many KB: the streamed form
  static constexpr int ISNT = 4;  // the streamed form: at most 8 ISNT re-observed landmarks per walk over the panel
  static constexpr int kRec = ArrowWs::kRec;  // doubles per factor record (REC, k_slam_common.hip)
  static INC_CARVE_FN size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

  int Lcap = 0, n1 = 0, n1p = 0, a0 = 0, ldw = 0, ncap = 0;
  size_t plan_off = 0;
  size_t fre = 0, fnew = 0, fslot = 0, ictl = 0, fq = 0, recs = 0, gs = 0, vvec = 0, wks = 0, thp = 0, thl = 0, dl = 0, Dl = 0, Y = 0, cwl = 0, Yh = 0;
  size_t fixed = 0;        // what the plan needs whatever the form: plan_off + everything up to and including Y
  bool feasible = false;   // fixed <= lds_bytes; false: the step cannot take this path, the update is a full solve
  bool lds_panel = false;  // the panel is staged in LDS for the step
  bool wide = false;       // room for the second half of Y: batches of up to 16 re-observed landmarks
  // the streamed form (the pose-chain solver's kernels, the panel in HBM / L2): snt factor tiles per walk (0: not this form)
  int snt = 0, yrows = 0;
  size_t yt = 0, wim = 0, jt = 0, svv = 0;

  // bytes of the streamed form's images behind x.Y at t tiles per walk: Y^T (t tiles), the images 5 .. t^2 - 1 of W', the batch's
  // Jacobians, the vectors
  static INC_CARVE_FN size_t stream_bytes(int t, int yrows) {
    return (size_t)t * yrows * IYS * 8 + (size_t)(t * t - 5 > 0 ? t * t - 5 : 0) * 16 * IYS * 8 + (size_t)16 * t * 8 * 8 + 64 * 8;
  }

  INC_CARVE_FN IncCarve(int P, int L0, int L_max, size_t sim_lds, size_t lds_bytes, size_t smem_off) {
    Lcap = L_max < L0 + INEW ? L_max : L0 + INEW;
    n1 = 3 * P + 2 * L0; n1p = (n1 + 15) & ~15;
    a0 = 3 + 2 * L0;
    ldw = (3 + 2 * Lcap + 31) & ~31;  // (whole pairs of 16-column tiles: inc_post, B3)
    ncap = 3 * P + 2 * Lcap > n1p ? 3 * P + 2 * Lcap : n1p;
    plan_off = sim_lds;
    // (no fused kernel ever serves this state - more poses than the dense solver takes and more landmarks than k_step_arrow sweeps in
    // LDS, drlgx_step_arrow_fusable -: nothing to agree with, the simulator's region is not set aside)
    if ((3 * P + 1 + 15) / 16 > kDenseTiles && 2 * L_max + 1 > 16 * kFastTilesArrow) plan_off = 0;
    if (smem_off > plan_off) plan_off = smem_off;
    size_t off = up16(smem_off);
    const size_t off0 = off;
    fre = off; off += up16(INF * 4);      // re-observed: index (0 .. nf-1) of the factor, in factor order
    fnew = off; off += up16(INF * 4);     // new landmark L0 + j: index of its factor
    fslot = off; off += up16(INF * 4);    // landmark slot of factor t
    ictl = off; off += up16(16);          // [0] re-observed count, [1] numerical flag (inv16_blk), [2] structure flag
    fq = off; off += up16(32 * 8);                  // F (9), c (3), theta of the new pose (4), measured odometry (4)
    recs = off; off += up16(INF * kRec * 8);        // linearised new factors
    gs = off; off += up16(INEW * 12 * 8);           // per new landmark: G (6), c (2), Q (xx xy yy), pad
    vvec = off; off += up16(32 * 8);
    wks = off; off += up16(5 * 16 * IYS * 8);       // W' as operand images: one tile, or four + a transposition scratch
    thp = off; off += up16((size_t)P * 4 * 8);
    thl = off; off += up16((size_t)Lcap * 2 * 8);
    dl = off; off += up16((size_t)ncap * 8);        // delta, logical row order
    Dl = off; off += up16((size_t)P * 6 * 8);
    Y = off; off += up16((size_t)(n1p + 1) * IYS * 8);  // (+ one row of zeros: the pad columns' operand)
    cwl = off;
    fixed = up16(plan_off) + (off - off0);
    feasible = fixed <= lds_bytes;
    lds_panel = fixed + (size_t)ncap * ldw * 8 <= lds_bytes;
    // the second half of Y (wide batches) sits behind the panel, if there is room left
    const size_t pan = lds_panel ? (size_t)ncap * ldw * 8 : 0, yh = (size_t)(n1p + 1) * IYS * 8;
    Yh = cwl + pan;
    wide = fixed + pan + yh <= lds_bytes;
    // (the dense solver's kernels - k_step, k_slam: <= 53 poses - keep the two-walk form for the panels that miss the LDS: those are a
    // few hundred KB that stay in L2, and the streamed form's fixed costs - a k x k inverse, the gathers at the head of every row tile -
    // made the 48-landmark instance of the bench state 6 us slower)
    if (feasible && !lds_panel && (3 * P + 1 + 15) / 16 > kDenseTiles) {
      // The panel stays in HBM / L2: the update walks it ONCE per batch of up to 8 snt landmarks (inc_stream_batch), and what it
      // keeps in LDS is indexed by the panel's COLUMNS, not its rows: Y^T of the active variables as snt tiles of 16 factor columns
      // (rows = the columns of the panel + one row of zeros for the pad columns), the snt x snt operand images of
      // W' = -T^-1 and the batch's Jacobians in column order - everything from Y to the end of the LDS.
      yrows = a0 + 1;  // (+ one row of zeros: the operand of the pad columns)
      // (sized like everything else in this plan: as if the carve began at plan_off - the fused step and the stage kernels agree)
      const size_t avail = lds_bytes - (up16(plan_off) + (Y - off0));
      for (int t = ISNT; t >= 1 && !snt; --t)
        if (stream_bytes(t, yrows) <= avail) snt = t;
      yt = Y;
      wim = yt + (size_t)snt * yrows * IYS * 8;  // images 5 .. snt^2 - 1 of W' (the first five: wks)
      jt = wim + (size_t)(snt * snt - 5 > 0 ? snt * snt - 5 : 0) * 16 * IYS * 8;
      svv = jt + (size_t)16 * snt * 8 * 8;
    }
  }
};

// Which form serves an update of n_re re-observed landmarks (inc_post): the streamed one where it exists (snt > 0) unless the
// two-walk form needs a single batch and the panel is small enough for L2 to serve its second walk.
INC_CARVE_FN bool inc_streams(int snt, bool wide, int n_re, int n1, int a0) {
  return snt > 0 && (n_re > (wide ? 16 : 8) || (size_t)n1 * a0 * 8 > (size_t)(IncCarve::kStreamKB << 10));
}
// streamed form: factor tiles (of 8 landmarks) of the next walk when `left` landmarks remain
INC_CARVE_FN int inc_stream_tiles(int snt, int left) { return snt < (left + 7) >> 3 ? snt : (left + 7) >> 3; }
// the other forms: is the next batch a wide one (up to 16 landmarks) or a narrow one (up to 8)?
INC_CARVE_FN bool inc_batch_wide(bool wide, int left) { return left > 8 && wide; }

// anchors: forms DESIGN.md states for the small world of tests/step_cases.py (63 landmarks at most, 160 KB of LDS, the simulator's
// region of 190 listed landmarks: 11 904 B) - the ring of 33 at 3 poses, and with its gate of 13 at 6
static_assert(IncCarve(3, 33, 63, 11904, 160 * 1024, 0).lds_panel && IncCarve(3, 33, 63, 11904, 160 * 1024, 0).wide, "lds wide");
static_assert(!IncCarve(6, 46, 63, 11904, 160 * 1024, 0).lds_panel && IncCarve(6, 46, 63, 11904, 160 * 1024, 0).wide, "two-walk wide");
static_assert(IncCarve(54, 17, 63, 11904, 160 * 1024, 0).snt == 4 && inc_streams(4, true, 17, 196, 37) && inc_stream_tiles(4, 17) == 3, "streamed 3");

#undef INC_CARVE_FN
}  // namespace kslam
