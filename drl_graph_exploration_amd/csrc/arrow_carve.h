// Memory layout of the pose-chain solver (k_slam_arrow.hip: arrow_body): the ONE place that says where each of its arrays lies,
// in the dynamic LDS (ArrowCarve) and in the per-instance HBM workspace (ArrowWs), and how much of either an engine needs.  The
// kernel takes its pointers from it; the host (k_slam_host.hip) sizes the workspace and admits capacities from it.
// Plain C++ (constexpr functions are host and device functions to the HIP compiler): a host program can include it alone.
#pragma once
#include <stddef.h>

namespace kslam {

#define ARROW_CARVE_FN constexpr __attribute__((always_inline))  // (also inside the kernels: no call)
constexpr int kSegLog = 3, kSeg = 1 << kSegLog;  // leaf segments of the chain: 7 interior poses between separators
// The landmark system: <= 63 landmarks (N <= 128) packed in LDS; beyond, swept from the workspace with up to kArrowRegTiles
// register tiles per wave (N <= 256, <= 127 landmarks) or, larger still, every tile streamed (k_sweep_ws.hip)
constexpr int kFastTilesArrow = 8;
constexpr int kArrowRegTiles = 20;

ARROW_CARVE_FN size_t arrow_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }
// row stride of X = T^-1 [B eta_p (E_pn)] for L landmarks: 2L + 1 columns, room for the three unit columns of the newest pose
// whether they are used or not, rounded to 32-byte rows
ARROW_CARVE_FN int arrow_ldx(int L) { return (2 * L + 1 + 3 + 3) & ~3; }
// doubles of the packed landmark system's LDS region (N <= 16 kFastTilesArrow): the triangle or the sweep panels that alias it.
// This is sweep_region_doubles (k_sweep.hip), which says what sweep_packed_fast writes; k_slam_arrow.hip asserts the two equal
// at every N the solver packs, so a change there that is not made here does not compile
ARROW_CARVE_FN size_t arrow_packed_doubles(size_t N) {
  const size_t tri = N * (N + 1) / 2 + 6 * N + 64, pan = 64 * N + 1024;
  return tri > pan ? tri : pan;
}
// doubles of the LDS region of the landmark system of N = 16 Tn rows: packed, the panels of the register-tile sweep, or the
// E tiles and scratch of the streamed one.  NTW: register tiles per wave the kernel was compiled with; kWaves - 1 = 7 waves hold tiles.
ARROW_CARVE_FN size_t arrow_sys_doubles(size_t N, int NTW) {
  const size_t Tn = N / 16;
  return Tn <= (size_t)kFastTilesArrow ? arrow_packed_doubles(N) : NTW > 0 && Tn * (Tn + 1) / 2 <= (size_t)NTW * 7 ? 32 * N + 1280 : 1280;
}

// Workspace of one instance for capacities (P_max, L_max, M_max).  All members: offsets in doubles.
struct ArrowWs {
  static constexpr int kRec = 12;  // doubles per factor record (REC, k_slam_common.hip)
  size_t X = 0;      // [3 P][ldx] T^-1 [B eta_p (E_pn)]
  size_t Ti = 0;     // [P][6] (T^-1)_ii, symmetric
  size_t Sl = 0;     // [P][9] (T^-1)_{i-s,i} at i's elimination level
  size_t Sr = 0;     // [P][9] (T^-1)_{i+s,i}
  size_t sepR = 0;   // [P / kSeg + 2][3][ldx] leaf -> right separator rhs
  size_t rec = 0;    // [M][kRec] the factor records when the LDS does not hold them
  size_t A = 0;      // [2 L + 17][2 L + 17] the square landmark system beyond 63 landmarks
  size_t pws = 0;    // [32][2 L + 17] panels of the streamed sweep
  size_t obs = 0;    // u16 [L][P] the observation table when the LDS does not hold it
  size_t total = 0;  // all of it; instances stay 256-byte aligned: 32-byte row loads of X

  ARROW_CARVE_FN ArrowWs(int P_max, int L_max, int M_max) {
    const size_t P = (size_t)P_max, ldx = (size_t)arrow_ldx(L_max), n = (size_t)(2 * L_max + 17);
    Ti = X + 3 * P * ldx;
    Sl = Ti + 6 * P;
    Sr = Sl + 9 * P;
    sepR = Sr + 9 * P;
    rec = sepR + (size_t)(P_max / kSeg + 2) * 3 * ldx;
    A = rec + (size_t)M_max * kRec;
    pws = A + n * n;
    obs = pws + 32 * n;
    total = arrow_up(obs + ((size_t)L_max * P * 2 + 7) / 8 + 16, 32);
  }
};

// LDS of one solve: P poses, L landmarks, M factors (the actual counts), by the kernel instantiation NTW in lds_bytes of
// dynamic LDS; mk_panel: the chain solve carries the three unit columns of the newest pose.  All offsets in bytes.
struct ArrowCarve {
  static constexpr int kThp = 4, kDd = 6, kAl = 9, kGL = 9, kGR = 9;  // doubles per pose of the chain tables
  static constexpr int kThl = 2, kLamb = 8;                          // doubles per landmark
  // bytes of the per-pose / per-landmark tables (everything in front of the union region)
  static ARROW_CARVE_FN size_t tables_bytes(int P, int L) {
    return (size_t)P * (kThp + kDd + kAl + kGL + kGR) * 8 + (size_t)L * (kThl + kLamb) * 8 + arrow_up((size_t)(P + 2) * 4, 8) + 8 +
           (size_t)L * (((size_t)P + 63) >> 6) * 8;
  }
  // LDS the solver cannot do without at capacity: the tables and the landmark system (the observation table, the separator
  // rows and the factor records overflow to the workspace); 120 bytes cover the alignment of the regions
  static ARROW_CARVE_FN size_t min_bytes(int P_max, int L_max) {
    const size_t N = 16 * (((size_t)2 * L_max + 1 + 15) / 16);
    return tables_bytes(P_max, L_max) + arrow_sys_doubles(N, kArrowRegTiles) * 8 + 120;
  }

  int np = 0, ncol = 0, ncx = 0, ldx = 0;  // landmark system: pivots [0, 2L), rhs row 2L; columns of [B eta_p (E_pn)]; row stride of X
  int Tn = 0, N = 0, MW = 0, nsep = 0;     // tile rows, N = 16 Tn; mask words per landmark; separators (= leaf segments)
  bool c_lds = false, c_reg = false;       // system packed in LDS / lower tiles in registers, panels in LDS / neither: streamed
  size_t thp = 0;     // double [P][4] theta
  size_t Dd = 0;      // double [P][6] D_i (symmetric) -> E_i = its inverse when i is eliminated
  size_t Al = 0;      // double [P][9] A_i = T_{i,i-s}: coupling to the current left neighbour
  size_t GL = 0;      // double [P][9] E_i A_i
  size_t GR = 0;      // double [P][9] E_i A_{i+s}^T
  size_t thl = 0;     // double [L][2]
  size_t lamb = 0;    // double [L][8] Lambda_jj (3), eta_j at [6..7]
  size_t mstart = 0;  // int [P + 2] first factor of each pose
  size_t bad = 0;     // int: a pivot was not positive
  size_t lmask = 0;   // u64 [L][MW] poses that observe the landmark
  size_t obs = 0;     // u16 [L][P] factor index + 1 (obs_lds)
  size_t U = 0;       // union region: the separators' rhs rows (xs_lds) during the chain solve, then the landmark system
  size_t rec = 0;     // double [M][kRec] factor records (rec_lds)
  bool obs_lds = false, xs_lds = false, rec_lds = false;  // what fits the LDS; otherwise in the workspace (xs: in X itself)
  size_t u_free = 0;  // bytes from U on that are free once the union region's contents are dead: up to rec if it lives in LDS
  size_t end = 0;     // end of the carve

  ARROW_CARVE_FN ArrowCarve(int P, int L, int M, int NTW, int lds_bytes, bool mk_panel) {
    np = 2 * L; ncol = np + 1;
    ncx = mk_panel ? ncol + 3 : ncol;
    ldx = arrow_ldx(L);
    Tn = (ncol + 15) / 16; N = 16 * Tn;
    MW = (P + 63) >> 6;
    nsep = (P + kSeg - 1) / kSeg;
    c_lds = Tn <= kFastTilesArrow;
    c_reg = !c_lds && NTW > 0 && Tn * (Tn + 1) / 2 <= NTW * 7;
    const size_t nP = (size_t)P, nL = (size_t)L, lds = (size_t)lds_bytes;
    Dd = thp + nP * kThp * 8;
    Al = Dd + nP * kDd * 8;
    GL = Al + nP * kAl * 8;
    GR = GL + nP * kGL * 8;
    thl = GR + nP * kGR * 8;
    lamb = thl + nL * kThl * 8;
    mstart = lamb + nL * kLamb * 8;
    bad = mstart + arrow_up((size_t)(P + 2) * 4, 8);
    lmask = bad + 8;
    size_t off = arrow_up(lmask + nL * MW * 8, 32);
    const size_t sys_bytes = arrow_sys_doubles((size_t)N, NTW) * 8, obs_bytes = arrow_up(nL * P * 2, 8);
    obs_lds = off + sys_bytes + obs_bytes + 32 <= lds;
    obs = off;
    if (obs_lds) off += arrow_up(obs_bytes, 32);
    U = off;
    const size_t xs_bytes = (size_t)nsep * 3 * ldx * 8;
    xs_lds = off + (sys_bytes > xs_bytes ? sys_bytes : xs_bytes) <= lds;
    off += xs_lds && xs_bytes > sys_bytes ? xs_bytes : sys_bytes;
    rec = off;
    rec_lds = off + (size_t)M * ArrowWs::kRec * 8 <= lds;
    u_free = rec_lds ? off - U : lds - U;
    if (rec_lds) off += (size_t)M * ArrowWs::kRec * 8;
    end = off;
  }
};

// anchors: the workspace and the LDS minimum at capacities the project uses, by the formulas these structs replaced
static_assert(ArrowWs(127, 127, 3800).total == 247136 && ArrowCarve::min_bytes(127, 127) == 126208, "bench.py's config 5 moved");
static_assert(ArrowWs(80, 500, 3600).total == 1399104 && ArrowCarve::min_bytes(80, 500) == 82376, "the 500-landmark engine moved");
static_assert(ArrowWs(41, 8, 492).total == 12032 && ArrowCarve::min_bytes(41, 8) == 37720, "the default engine (41 poses, 40 m map) moved");
static_assert(ArrowWs(41, 100, 512).total == 91584 && ArrowCarve::min_bytes(41, 100) == 84728, "bench.py's 41-pose engine moved");

// The forms of phase 10, the pose products (ArrowCtx::pose_products, products_staged), as the kernel and the host's
// drlgx_debug_arrow_form decide them.  np = 2 L pivots in nK = (np + 15) / 16 chunks of the product's K dimension.
constexpr int kArrowPanelChunks = 8;  // K chunks whose 16-row panel of X a wave holds in registers (products_tiles)
constexpr int kArrowZG = 3;           // column tiles per group of the staged form, at most
ARROW_CARVE_FN bool arrow_products_vector(bool c_lds, int np) { return c_lds && np <= 12; }
ARROW_CARVE_FN bool arrow_products_tiles(int np) { return (np + 15) / 16 <= kArrowPanelChunks; }  // (else staged)
// staged form: as many column tiles per group as the LDS behind the pose tables holds (one tile = nK x 2 KB); none: one tile,
// staged in the workspace's sweep panels
ARROW_CARVE_FN int arrow_zfit(size_t u_free, int nK) { return (int)(u_free / ((size_t)nK * 2048)); }
ARROW_CARVE_FN int arrow_zg(int zfit) { return zfit >= 1 ? (kArrowZG < zfit ? kArrowZG : zfit) : 1; }

#undef ARROW_CARVE_FN
}  // namespace kslam
