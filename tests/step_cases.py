"""TEST INFRASTRUCTURE: the worlds at which the loops of the belief step wrap - ksim::scan_in_range / measure / draw_normals
(csrc/k_sim.hip) at 63 .. 130 landmarks in range, the incremental update's batches and fallbacks (csrc/k_inc.hip) at 8 .. 65
re-observed landmarks, 64 / 65 new factors and 12 / 13 first sightings - shared by tests/test_step_cpu.py (which proves on the
CPU, with the oracle alone, that the worlds are what they claim) and tests/test_gpu_step_edges.py (which runs them on the device).

Listed landmarks only.  Environment e starts at the centre of ring e, off the integer lattice, heading away from the other row of
rings.  A ring is two arcs of 2 m radius, left and right of the vehicle's axis, that leave 50 degrees behind it empty (no landmark
ever comes near the +-179.9 degree bearing gate) and 40 degrees ahead (the gate move ends on the circle); the centres lie on a 9.5 m
grid, so another ring's nearest landmark is 7.5 m from a centre.  A ring may carry a GATE CLUSTER of m landmarks 7.5 m ahead of its
centre: out of range from the centre, about 5.5 m away after a 2 m forward move.

The simulator's translation noise would let the ground truth wander off over 57 steps, so the scripts are closed-loop ON THE
ORACLE's ground truth: a jiggle is a small body-frame move back towards the centre and the start heading plus an alternating
+-0.05 m / +-0.01 rad.  The actions are computed from the oracles step by step and handed to the engine as they are: both sides
execute the same numbers.  The two worlds of the incremental update also change three config values (INC_TUNE, with the reason).

Steps are numbered from 0 (the first move); the reset is step -1.  After step s an environment holds s + 2 poses and has run
s + 2 iSAM updates, so the updates that may relinearise (every 10th) are steps 8, 18, 28, 38 and 48.
"""
import math

import numpy as np

from oracle import oracle as O

MAP = 40
GRID = 9.5
RADIUS = 2.0
GAP_DEG = 25.0                 # half-width of the empty arc behind the vehicle
AHEAD_DEG = 20.0               # ... and of the one ahead of it: the 2 m gate move ends ON the circle, 0.69 m from the nearest landmark
GATE_AHEAD = 7.5
GATE_MOVE = 2.0
GATE_SPACING = 0.02            # rad between neighbours of a gate cluster, seen from the centre
JIG_CLIP, JIG_AMP, JIG_ROT = 0.25, 0.05, 0.01
MAX_RANGE_MARGIN = 1.0         # no foreign landmark within max_range + this of any ground-truth pose

# kernel constants the tables below restate (csrc/k_inc.hip, k_slam_common.hip, slam_carve.h, drlgx_dev.h)
INF, INEW, ISNT, IYS, REC = 64, 12, 4, 18, 12
LDS_BUDGET, DENSE_TILES, MT_STRIDE, STREAM_KB = 160 * 1024, 10, 626, 512
DENSE_MAX_POSES = 53           # (3 P + 1 + 15) / 16 <= kDenseTiles

SHORT = "jjgbgb"               # 7 poses: the dense kernels
LONG = "j" * 53 + "gbgb"       # 58 poses: from step 52 (54 poses) on the pose-chain kernels; the gate is first seen at step 53
SIM_SCRIPT = "jjj"
LONG_CHECKS = (0, 7, 8, 9, 30, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56)  # 51 / 52: either side of pose 54; 53, 55: the gate steps
LONG_SOLO = (51, 52, 53, 54, 55, 56)  # stepped one environment at a time: inc_stats attributable


def _slot(col, row):
    """Centre and heading of grid slot (col 0 .. 3, row 0 = bottom / 1 = top): the two outer rows of the 4 x 4 grid, heading outwards."""
    x = -1.5 * GRID + GRID * col + 0.3183
    y = (1.5 * GRID if row else -1.5 * GRID) - 0.2718
    th = (math.pi / 2 if row else -math.pi / 2) + 0.0234 * (1 + col) * (1 if (col + row) % 2 else -1)
    return x, y, th


class World(object):
    """rings: [(size, gate size or 0)], environment e in grid slot e (row-major).  `fixed`: ring after ring, a ring's gate directly
    behind it.  caps: the engine capacities."""

    def __init__(self, name, rings, caps, tune=None):
        self.name, self.rings, self.caps, self.tune = name, list(rings), dict(caps), dict(tune or {})
        self.n = len(rings)
        self.starts = np.array([_slot(e % 4, e // 4) for e in range(self.n)])
        pts, self.ring_keys, self.gate_keys = [], [], []
        k = 0
        for (size, gate), (cx, cy, th) in zip(self.rings, self.starts):
            nl, arc = (size + 1) // 2, math.radians(180 - GAP_DEG - AHEAD_DEG)   # two arcs: left of the axis, right of it
            beta = np.concatenate([math.radians(AHEAD_DEG) + (np.arange(nl) + 0.5) * arc / nl,
                                   -math.radians(AHEAD_DEG) - (np.arange(size - nl) + 0.5) * arc / max(size - nl, 1)])
            pts.append(np.stack([cx + RADIUS * np.cos(th + beta), cy + RADIUS * np.sin(th + beta)], axis=1))
            self.ring_keys.append(np.arange(k, k + size))
            k += size
            a = (np.arange(gate) - (gate - 1) / 2.0) * GATE_SPACING + 0.0037
            pts.append(np.stack([cx + GATE_AHEAD * np.cos(th + a), cy + GATE_AHEAD * np.sin(th + a)], axis=1))
            self.gate_keys.append(np.arange(k, k + gate))
            k += gate
        self.fixed = np.concatenate(pts)
        self.num_landmarks = len(self.fixed)

    def oracle_config(self):
        return self._tuned(O.default_config(MAP, num_landmarks=self.num_landmarks))

    def _tuned(self, cfg):
        for k, v in self.tune.items():
            setattr(cfg, k, v)
        return cfg

    def make_sims(self):
        ocfg = self.oracle_config()
        return [O.OracleSim(ocfg, e, e, start=tuple(self.starts[e]), fixed_landmarks=self.fixed) for e in range(self.n)]

    def engine_config(self, **override):
        from drl_graph_exploration_amd import default_config
        caps = dict(self.caps)
        caps.update(override)
        return self._tuned(default_config(MAP, num_landmarks=self.num_landmarks, **caps))

    # ---- the closed-loop scripts
    def action(self, sim, e, kind, s):
        """The action of environment e at step s of a script whose letter there is `kind`: j = jiggle, g = the 2 m gate move
        (gate rings only; a jiggle elsewhere), b = back to the centre."""
        if self.rings[e][1] == 0 and kind in "gb":
            kind = "j"
        if kind == "g":
            return (GATE_MOVE, 0.0, 0.0)
        veh = sim.ground_truth()[0]
        cx, cy, th0 = self.starts[e]
        dx, dy = cx - veh[0], cy - veh[1]
        d = math.hypot(dx, dy)
        clip = JIG_CLIP if kind == "j" else 3.0
        if d > clip:
            dx, dy = dx * clip / d, dy * clip / d
        c, sn = math.cos(veh[2]), math.sin(veh[2])
        sign = 1.0 if s % 2 == 0 else -1.0
        ox, oy = c * dx + sn * dy + sign * JIG_AMP, -sn * dx + c * dy
        oth = min(max(O.wrap_theta(th0 - veh[2]), -0.05), 0.05) + sign * JIG_ROT
        return (ox, oy, oth)

    def actions(self, sims, kind, s):
        return np.array([self.action(sims[e], e, kind, s) for e in range(self.n)], dtype=np.float64)

    # ---- what the worlds claim (asserted against the oracle by tests/test_step_cpu.py)
    def expected_counts(self, script):
        """[step + 1][environment] = (n_in, nf, n_re, nn): ground-truth landmarks in range, factors appended, landmarks
        re-observed, first sightings; row 0 is the reset."""
        rows = [[(size, size, 0, size) for size, _ in self.rings]]
        seen = [False] * self.n
        for kind in script:
            row = []
            for e, (size, gate) in enumerate(self.rings):
                if kind == "g" and gate:
                    row.append((size + gate, size + gate, size + (gate if seen[e] else 0), 0 if seen[e] else gate))
                    seen[e] = True
                else:
                    row.append((size, size, size, 0))
            rows.append(row)
        return rows


def expected_path(counts, update_no, relinearises):
    """'full' or 'inc' for one update (csrc/k_inc.hip: inc_precheck, inc_post's `feasible`): the reset's solve, an update that
    relinearises, more than INF new factors and more than INEW first sightings are full solves, everything else is a rank-k update."""
    n_in, nf, n_re, nn = counts
    if update_no == 1 or relinearises or nf > INF or nn > INEW:
        return "full"
    return "inc"


def relinearises(sim):
    """Will the NEXT update of this oracle relinearise?  (oracle/drlgx_oracle.cpp Isam::update: every 10th update, a variable
    whose |delta|_inf >= 0.1.)  Returns (bool, max |delta|)."""
    _, dp, _, dl, count = sim.isam_state()
    mx = max(np.abs(dp).max() if dp.size else 0.0, np.abs(dl).max() if dl.size else 0.0)
    return ((count + 1) % 10 == 0 and mx >= 0.1), float(mx)


# ---------------------------------------------------------------------------------------------------------------- the worlds
def sim_worlds():
    """The simulator's wraps.  num_landmarks <= 128: scan_in_range's prefetch form; above: its loop form.  n_in >= 129: the
    trip of measure() that no longer reads prefetched registers."""
    mk = lambda name, sizes: World(name, [(s, 0) for s in sizes], dict(  # noqa: E731
        max_poses=8, max_landmarks=max(sizes), max_factors=8 * max(sizes), max_actions=4))
    return [mk("pre128", [128]), mk("pre65_63", [65, 63]), mk("pre64_63", [64, 63]),
            mk("loop129", [129]), mk("loop130", [130]), mk("loop128_64_65", [128, 64, 65])]


SIM_N_IN = {"pre128": [128], "pre65_63": [65, 63], "pre64_63": [64, 63], "loop129": [129], "loop130": [130], "loop128_64_65": [128, 64, 65]}

SMALL_RINGS = [(8, 1), (9, 0), (16, 0), (17, 12), (24, 0), (25, 0), (32, 0), (33, 13)]
LARGE_RINGS = [(48, 0), (52, 12), (63, 0), (64, 1), (65, 0)]


# The worlds of the incremental update run a quieter vehicle and a tighter prior than exploration_env.ini (both sides take the
# values from the config).  With the default 0.1 m of translation noise every new pose's delta crosses the relinearisation
# threshold, so every 10th update would be a full solve; with the default prior (0.05 m) the landmarks' marginals are dominated
# by the start pose's uncertainty, and a landmark seen 50 times no longer moves its block by 1000 tolerances.
INC_TUNE = dict(translation_noise=0.01, sigma_x0=0.02, sigma_y0=0.02)


def small_world():
    """L_max = 63: the fused pose-chain step serves it (2 L_max + 1 <= 128)."""
    return World("small", SMALL_RINGS, dict(max_poses=60, max_landmarks=63, max_factors=2048, max_actions=4), INC_TUNE)


def large_world():
    """L_max = 78: no fused pose-chain kernel serves it; beyond 53 poses the steps are the three stage kernels."""
    return World("large", LARGE_RINGS, dict(max_poses=60, max_landmarks=78, max_factors=3840, max_actions=4), INC_TUNE)


def capacity_world():
    """Ring 65 (with a 12-gate) beside ring 8; the capacities are the test's."""
    return World("capacity", [(65, 12), (8, 0)], dict(max_poses=8, max_landmarks=80, max_factors=1024, max_actions=4))


WORLDS = {"small": small_world, "large": large_world}
SCRIPTS = {"short": SHORT, "long": LONG}


# ------------------------------------------------------------------------ which form of the update serves a case (k_inc.hip)
def _up16(b):
    return (b + 15) & ~15


def sim_lds_bytes(LG, pc, P_max):
    """drlgx_sim_lds_bytes (csrc/drlgx_dev.h) as inc_plan calls it: with the launch's pose bound pc for its pose argument (so the pose
    tables count up to pc = 64 whatever max_poses is; P_max is not part of it)."""
    b = 2 * MT_STRIDE * 4 + (2 * LG + 2) * 8 + LG * 4 + 16
    b = ((b + 7) & ~7) + 2 * LG * 8
    if pc <= 64:
        b = max(b, pc * 19 * 8 + 32)
    return (b + 31) & ~31


def inc_form(P, L0, n_re, LG, P_max, L_max, pc=None):
    """The form inc_plan / inc_post choose for the update that brings an instance to P poses with L0 landmarks in the panel and
    n_re re-observed landmarks - a restatement of their arithmetic (not observable from outside the kernel):
      'lds narrow' / 'lds wide'          the panel staged in LDS, batches of <= 8 / <= 16 landmarks
      'two-walk narrow' / 'two-walk wide' the panel in HBM / L2, the same batches
      'streamed a+b+..'                   the panel in HBM / L2 walked once per batch of a, b, .. tiles of 8 landmarks."""
    pc = P if pc is None else pc
    Lcap = min(L_max, L0 + INEW)
    n1 = 3 * P + 2 * L0
    n1p = (n1 + 15) & ~15
    a0 = 3 + 2 * L0
    ldw = (3 + 2 * Lcap + 31) & ~31
    ncap = max(3 * P + 2 * Lcap, n1p)
    arrow = P > DENSE_MAX_POSES
    plan_off = 0 if (arrow and 2 * L_max + 1 > 128) else sim_lds_bytes(LG, pc, P_max)
    before_y = sum(_up16(b) for b in (INF * 4, INF * 4, INF * 4, 16, 32 * 8, INF * REC * 8, INEW * 12 * 8, 32 * 8, 5 * 16 * IYS * 8,
                                      P * 4 * 8, Lcap * 2 * 8, ncap * 8, P * 6 * 8))
    yh = (n1p + 1) * IYS * 8
    fixed = _up16(plan_off) + before_y + _up16(yh)
    if fixed > LDS_BUDGET:
        return "none"
    lds_panel = fixed + ncap * ldw * 8 <= LDS_BUDGET
    pan = ncap * ldw * 8 if lds_panel else 0
    wide = fixed + pan + yh <= LDS_BUDGET
    snt = 0
    if not lds_panel and arrow:
        avail = LDS_BUDGET - (_up16(plan_off) + before_y)
        yrows = a0 + 1
        for t in range(ISNT, 0, -1):
            if t * yrows * IYS * 8 + max(0, t * t - 5) * 16 * IYS * 8 + 16 * t * 8 * 8 + 64 * 8 <= avail:
                snt = t
                break
    if not lds_panel and arrow and snt > 0 and (n_re > (16 if wide else 8) or n1 * a0 * 8 > (STREAM_KB << 10)):
        tiles, left = [], n_re
        while left > 0:
            nt = min(snt, (left + 7) >> 3)
            tiles.append(nt)
            left -= min(8 * nt, left)
        return "streamed " + "+".join(str(t) for t in tiles)
    return ("lds " if lds_panel else "two-walk ") + ("wide" if wide else "narrow")


def form_table(world, script):
    """{(ring size, step): form} for the jiggle step 1 (short: 3 poses; long: step 54 is taken instead, 56 poses, the step behind
    the first gate step) and the gate steps of a script, for every ring whose update is served incrementally there."""
    counts = world.expected_counts(script)
    out = {}
    steps = [s for s, k in enumerate(script) if k == "g"] + ([1] if len(script) < 10 else [52, 54])
    for s in sorted(steps):
        for e, (size, gate) in enumerate(world.rings):
            n_in, nf, n_re, nn = counts[s + 1][e]
            if nf > INF or nn > INEW:
                continue
            L0 = size + (gate if any(script[t] == "g" for t in range(s)) else 0)
            out[(size, s)] = inc_form(s + 2, L0, n_re, world.num_landmarks, world.caps["max_poses"], world.caps["max_landmarks"])
    return out


# The table DESIGN.md states (k_inc): {world: {script: {(ring, step): form}}}, asserted against form_table() on the CPU.
FORMS = {
    "small": {
        "short": {
            (8, 1): "lds wide", (9, 1): "lds wide", (16, 1): "lds wide", (17, 1): "lds wide", (24, 1): "lds wide", (25, 1): "lds wide", (32, 1): "lds wide", (33, 1): "lds wide",
            (8, 2): "lds wide", (9, 2): "lds wide", (16, 2): "lds wide", (17, 2): "lds wide", (24, 2): "lds wide", (25, 2): "lds wide", (32, 2): "lds wide",
            (8, 4): "lds wide", (9, 4): "lds wide", (16, 4): "lds wide", (17, 4): "lds wide", (24, 4): "lds wide", (25, 4): "lds wide", (32, 4): "lds wide", (33, 4): "two-walk wide",
        },
        "long": {
            (8, 52): "two-walk wide", (9, 52): "two-walk wide", (16, 52): "two-walk wide", (17, 52): "streamed 3", (24, 52): "streamed 3", (25, 52): "streamed 4", (32, 52): "streamed 4", (33, 52): "streamed 4+1",
            (8, 53): "two-walk wide", (9, 53): "two-walk wide", (16, 53): "two-walk wide", (17, 53): "streamed 3", (24, 53): "streamed 3", (25, 53): "streamed 4", (32, 53): "streamed 4",
            (8, 54): "two-walk wide", (9, 54): "two-walk wide", (16, 54): "two-walk wide", (17, 54): "streamed 3", (24, 54): "streamed 3", (25, 54): "streamed 4", (32, 54): "streamed 4", (33, 54): "streamed 4+1",
            (8, 55): "two-walk wide", (9, 55): "two-walk wide", (16, 55): "two-walk wide", (17, 55): "streamed 4", (24, 55): "streamed 3", (25, 55): "streamed 4", (32, 55): "streamed 4", (33, 55): "streamed 4+2",
        },
    },
    "large": {
        "short": {
            (48, 1): "two-walk wide", (52, 1): "two-walk wide", (63, 1): "two-walk wide", (64, 1): "two-walk wide",
            (48, 2): "two-walk wide", (52, 2): "two-walk wide", (63, 2): "two-walk wide",
            (48, 4): "two-walk wide", (52, 4): "two-walk wide", (63, 4): "two-walk wide",
        },
        "long": {
            (48, 52): "streamed 4+2", (52, 52): "streamed 4+3", (63, 52): "streamed 4+4", (64, 52): "streamed 4+4",
            (48, 53): "streamed 4+2", (52, 53): "streamed 4+3", (63, 53): "streamed 4+4",
            (48, 54): "streamed 4+2", (52, 54): "streamed 4+3", (63, 54): "streamed 4+4", (64, 54): "streamed 4+4",
            (48, 55): "streamed 4+2", (52, 55): "streamed 4+4", (63, 55): "streamed 4+4",
        },
    },
}
