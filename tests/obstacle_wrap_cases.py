"""TEST INFRASTRUCTURE: two worlds of listed landmarks on which the in-range list of SS2D.simulate's obstacle flag (ksim::measure<kObs>,
ksim::scan_in_range; oracle/drlgx_oracle.cpp Env::simulate, return code 2) wraps its trips of 64 - in the style of
tests/obstacle_cases.py, shared by tests/test_obstacle_wrap_cpu.py (which proves on the CPU, with the oracle alone, that the worlds
are what they claim) and tests/test_gpu_obstacle_wrap.py (which runs them on the device).

The quiet vehicle, the +-120 degree sensor and safe_distance = 1.0 are obstacle_cases.TUNE.  Scripts are closed-loop on the ORACLE's
ground truth: the action of a step is the body-frame move from the oracle's true pose to the step's way point (a point relative to
the environment's centre and a heading), or 'R', an odometry outside the map box.

A PLACE is the 1-based position of a landmark in the in-range list in libstdc++'s hash iteration order: places 1-64 are the hit
loop's first trip, 65-128 its second (both served by the two-per-lane prefetch registers), 129 and beyond the third, which reads
inr[], gl[] and key_slot[] directly.  Places are fixed by handing an environment's points to its keys in iteration order
(orc_landmark_iteration_order).

WORLD W: three environments 13 m apart, six steps, LG = 325 (> 128: scan_in_range's generic loop).  Each has a near landmark K 0.6 m
ahead of its centre and N 0.6 m behind it, pads on an arc of 2.5 m BEHIND the centre (+-45 degrees about the rear axis: outside the
bearing gate by 15 degrees and more while the vehicle heads along +x, so they add to n_in and to nothing else; straight ahead after
the turn 't'), and - X, Y - two pads F1, F2 on the rear axis that leave the range gate when the vehicle drives ahead to 'u', 'v'.

  way points: c centre, heading 0   t centre, heading pi   u 1.85 m ahead, heading 0   v 3.0 m ahead, heading 0

  env  in range at the centre          script  codes   n_in per step        what it shows
  X    61 pads, F1, F2, K@64, N@65     cttt uv  220200  65 65 65 65 64 63    a hit at place 64 with an empty-handed second trip; a NEW
                                                                             landmark at place 65 with the latch down; n_in 63 / 64 / 65
  Y    126 pads, F1, K@128, N@129, F2  cttt uv  220200  130 x 4, 129, 128    a hit at place 128; at place 129 a NEW near landmark with
                                                                             the latch down (flags, step 1), the same landmark KNOWN with
                                                                             the latch down (does not, step 2), re-armed (step 3)
  Z    128 pads, N@129, K@130 (last)   cccRtt   202120  130 x 6              a hit at the last place; K known at place 130 with the latch
                                                                             down does not flag (step 1) while N - never sighted, too
                                                                             close, place 129 - is outside the bearing gate: no flag at
                                                                             steps 1 and 3; a rejected odometry between two flagged
                                                                             steps; N new with the latch down flags (step 4)

WORLD A: one environment, LG = 131, every listed landmark in range at every step (n_in == LG: the draw of 4 n_in variates fills the
opt-in's LDS carve to its end).  128 pads on an arc of 2.5 m AHEAD (+-45 degrees) and three near landmarks 0.6 m ahead (bearings -30,
0, 30 degrees) at places 10, 100 and 131: one in every trip at once.  It starts at the centre heading pi (everything behind it: the
reset's measure() sights nothing), turns to heading 0 (step 0: 131 first sightings in one call, flagged) and backs off 1.5 m (step 1:
clear)."""
import functools
import math

import numpy as np

import obstacle_cases as OC
from oracle import oracle as O

MAP, SAFE, MARGIN, TUNE = OC.MAP, OC.SAFE, OC.MARGIN, OC.TUNE
NEAR, ARC_R, ARC_HALF_DEG = 0.6, 2.5, 45.0
REJECT = OC.REJECT
HEADING = OC.HEADING
WAY = {"c": (0.0, 0.0, 0.0), "t": (0.0, 0.0, math.pi), "u": (1.85, 0.0, 0.0), "v": (3.0, 0.0, 0.0), "o": (-1.5, 0.0, 0.0)}
F1, F2 = (-5.0, 0.0), (-3.6, 0.0)


def _arc(n, about_deg):
    return [(ARC_R * math.cos(a), ARC_R * math.sin(a)) for a in np.radians(about_deg + np.linspace(-ARC_HALF_DEG, ARC_HALF_DEG, n))]


def _caps(states):
    """The smallest capacities the oracle's own counts need (landmarks to a multiple of 8, factors of 64; a pose more than the
    longest trajectory is not needed: a step only asks for P < max_poses before it)."""
    last = states[-1]
    up = lambda v, m: (v + m - 1) // m * m  # noqa: E731
    return dict(max_poses=max(s.num_poses() for s in last), max_landmarks=up(max(s.num_landmarks() for s in last), 8),
                max_factors=up(max(len(s.factors()[0]) for s in last), 64), max_actions=4)


class World(object):
    """names / scripts / codes / centres per env, blocks: per env the points (relative to its centre) in the ORDER OF THEIR PLACES."""

    def __init__(self, names, scripts, codes, centres, blocks, start_heading):
        self.names, self.scripts, self.codes, self.centres = names, scripts, codes, centres
        self.n, self.n_steps = len(names), len(scripts[0])
        self.starts = np.array([(cx, cy, O.wrap_theta(HEADING + start_heading)) for cx, cy in centres])
        self.keys, n = [], 0
        for b in blocks:
            self.keys.append(np.arange(n, n + len(b)))
            n += len(b)
        self.num_landmarks = n
        order = np.zeros(n, dtype=np.int32)
        O.lib().orc_landmark_iteration_order(n, order.ctypes.data_as(O.C.POINTER(O.C.c_int)))
        self.order = order
        self.fixed = np.zeros((n, 2))
        self.key_of = []  # [env][i]: the key that holds blocks[env][i]
        for e, b in enumerate(blocks):
            mine = set(int(k) for k in self.keys[e])
            in_order = [int(k) for k in order if int(k) in mine]
            for k, p in zip(in_order, b):
                self.fixed[k] = self.point(e, p)
            self.key_of.append(in_order)

    def point(self, e, p):
        cx, cy = self.centres[e]
        c, s = math.cos(HEADING), math.sin(HEADING)
        return (cx + c * p[0] - s * p[1], cy + s * p[0] + c * p[1])

    def _tuned(self, cfg):
        for k, v in TUNE.items():
            setattr(cfg, k, v)
        return cfg

    def oracle_config(self):
        return self._tuned(O.default_config(MAP, num_landmarks=self.num_landmarks))

    def make_sims(self):
        ocfg = self.oracle_config()
        return [O.OracleSim(ocfg, e, e, start=tuple(self.starts[e]), fixed_landmarks=self.fixed) for e in range(self.n)]

    def engine_config(self, caps, num_landmarks=None):
        from drl_graph_exploration_amd import default_config
        return self._tuned(default_config(MAP, num_landmarks=self.num_landmarks if num_landmarks is None else num_landmarks, **caps))

    def action(self, sim, e, kind):
        if kind == "R":
            return REJECT
        veh = sim.ground_truth()[0]
        wx, wy, wth = WAY[kind]
        tx, ty = self.point(e, (wx, wy))
        dx, dy = tx - veh[0], ty - veh[1]
        c, s = math.cos(veh[2]), math.sin(veh[2])
        return (c * dx + s * dy, -s * dx + c * dy, O.wrap_theta(HEADING + wth - veh[2]))


def _run(w):
    """The oracle's run of a world, once (obstacle_cases.reference's fields, plus caps)."""
    sims = w.make_sims()
    acts = np.zeros((w.n_steps, w.n, 3))
    codes = np.zeros((w.n_steps, w.n), dtype=np.int64)
    cleared = np.ones((w.n_steps, w.n), dtype=np.uint8)
    veh = np.zeros((w.n_steps, w.n, 3))
    latch = [True] * w.n
    states = [[sim.clone() for sim in sims]]  # states[0]: after the reset; states[s + 1]: after step s
    for s in range(w.n_steps):
        for e, sim in enumerate(sims):
            acts[s, e] = w.action(sim, e, w.scripts[e][s])
            codes[s, e] = sim.simulate(acts[s, e])
            if codes[s, e] != 1:
                latch[e] = codes[s, e] != 2
            cleared[s, e] = latch[e]
            veh[s, e] = sim.ground_truth()[0]
        states.append([sim.clone() for sim in sims])
    for a in (acts, codes, cleared, veh):
        a.setflags(write=False)
    return dict(actions=acts, codes=codes, flag=(codes == 2).astype(np.uint8), cleared=cleared, veh=veh, before=states[:-1],
                states=states[1:], caps=_caps(states))


W_NAMES = "XYZ"
W_SCRIPTS = ["ctttuv", "ctttuv", "cccRtt"]
W_CODES = ["220200", "220200", "202120"]
W_N_IN = [[65, 65, 65, 65, 64, 63], [130, 130, 130, 130, 129, 128], [130] * 6]
W_CENTRES = [(0.3183, -13.0 + 13.0 * e - 0.2718) for e in range(3)]  # (a column: every way point lies on an env's own x axis)
K, N = (NEAR, 0.0), (-NEAR, 0.0)
W_BLOCKS = [_arc(61, 180.0) + [F1, F2, K, N],
            _arc(126, 180.0) + [F1, K, N, F2],
            _arc(128, 180.0) + [N, K]]
W_PLACE = {("X", "K"): 64, ("X", "N"): 65, ("Y", "K"): 128, ("Y", "N"): 129, ("Z", "N"): 129, ("Z", "K"): 130}

A_PLACES = (10, 100, 131)
A_N_IN = [[131, 131]]


def _a_block():
    near = [(NEAR * math.cos(a), NEAR * math.sin(a)) for a in np.radians([-30.0, 0.0, 30.0])]
    b = _arc(128, 0.0)
    for p, q in zip(A_PLACES, near):
        b.insert(p - 1, q)
    return b


@functools.lru_cache(maxsize=None)
def world_w():
    return World(W_NAMES, W_SCRIPTS, W_CODES, W_CENTRES, W_BLOCKS, 0.0)


@functools.lru_cache(maxsize=None)
def world_a():
    return World("A", ["co"], ["20"], [W_CENTRES[1]], [_a_block()], math.pi)


@functools.lru_cache(maxsize=None)
def reference_w():
    return _run(world_w())


@functools.lru_cache(maxsize=None)
def reference_a():
    return _run(world_a())


def near_key(w, e, which):
    """The key of env e's K or N in world W."""
    b = W_BLOCKS[e]
    return w.key_of[e][b.index(K if which == "K" else N)]
