"""TEST INFRASTRUCTURE: one world of listed landmarks on which SS2D.simulate's obstacle flag (scripts/envs/pyss2d.py:132,180-197;
oracle/drlgx_oracle.cpp Env::simulate, return code 2) goes through every transition, shared by tests/test_obstacle_cpu.py (which
proves on the CPU, with the oracle alone, that the world is what it claims) and tests/test_gpu_obstacle.py (which runs it on the
device).

Six environments, six steps each.  Environment e lives around its own centre (13 m apart: no landmark of another environment is
ever in range), heading along +x; the sensor's field of view is narrowed to +-120 degrees (both sides take it from the config), so
that a landmark straight behind the vehicle is outside the bearing gate by 60 degrees, and the vehicle is quiet (translation noise
0.01 m), so that a landmark placed 0.6 m from a way point stays 0.4 m inside safe_distance = 1.0 - twenty range sigmas.  The
scripts are closed-loop on the ORACLE's ground truth (as tests/step_cases.py): the action of a step is the body-frame move from the
oracle's true pose to the step's way point - the centre, heading 0 ('c') or heading pi ('t', a turn on the spot) - or 'R': an
odometry outside the map box, which SS2D.simulate rejects.  Both sides execute the same numbers.

  env  landmarks (relative to the centre)                  script   codes    what it shows
  A    K ahead 0.6                                          cccccc   202020   clear -> hit, the latch held over a known landmark,
                                                                              the latch re-armed by the clear step
  B    K ahead 0.6, N behind 0.6                            cttttt   220202   hit -> hit on a NEW landmark with the latch down: N
                                                                              is first sighted in the very step it is too close
  C    G behind 0.5, F far                                  cccttt   000202   a close landmark outside the bearing gate does not count
  D    K ahead 0.6 + 65 on an arc of 2.5 m                  cccccc   202020   the hit's place in the in-range list is 65: K has the
                                                                              LAST of D's keys in hash iteration order
  E    K ahead 0.6, N behind 0.6                            cRtttt   212020   a rejected odometry between two flagged steps
  F    K ahead 0.6                                          cRcccc   210202   ... which leaves the latch alone: step 2 sees only K,
                                                                              known, with the latch still down
"""
import functools
import math

import numpy as np

from oracle import oracle as O

MAP = 40
SAFE = 1.0
MARGIN = 0.2                   # every true landmark distance stays this far from SAFE (ten range sigmas)
FOV_DEG = 120.0
TUNE = dict(safe_distance=SAFE, translation_noise=0.01, min_bearing=-math.radians(FOV_DEG), max_bearing=math.radians(FOV_DEG))
NEAR, ARC_R, ARC_N, ARC_HALF_DEG = 0.6, 2.5, 65, 100.0
REJECT = (100.0, 0.0, 0.0)     # x beyond map_max_x = 40: outside the map box
N_STEPS = 6

NAMES = "ABCDEF"
SCRIPTS = ["cccccc", "cttttt", "cccttt", "cccccc", "cRtttt", "cRcccc"]
CODES = ["202020", "220202", "000202", "202020", "212020", "210202"]   # orc_simulate: 0 stepped, 1 rejected, 2 obstacle
CENTRES = [(-19.5 + 13.0 * (e % 4) + 0.3183, (-10.0 if e < 4 else 10.0) - 0.2718) for e in range(6)]
HEADING = 0.0234
CAPS = dict(max_poses=8, max_landmarks=72, max_factors=1024, max_actions=4)


def _rel(e, pts):
    cx, cy = CENTRES[e]
    c, s = math.cos(HEADING), math.sin(HEADING)
    return [(cx + c * x - s * y, cy + s * x + c * y) for x, y in pts]


class World(object):
    def __init__(self):
        self.n = len(NAMES)
        self.starts = np.array([(cx, cy, HEADING) for cx, cy in CENTRES])
        arc = [(ARC_R * math.cos(a), ARC_R * math.sin(a))
               for a in np.radians(np.linspace(-ARC_HALF_DEG, ARC_HALF_DEG, ARC_N))]
        blocks = [[(NEAR, 0.0)],                       # A
                  [(NEAR, 0.0), (-NEAR, 0.0)],         # B
                  [(-0.5, 0.0), (3.0, 1.0)],           # C
                  arc + [(NEAR, 0.0)],                 # D (the near one: moved to D's last key in iteration order below)
                  [(NEAR, 0.0), (-NEAR, 0.0)],         # E
                  [(NEAR, 0.0)]]                       # F
        pts, self.keys = [], []
        for e, b in enumerate(blocks):
            self.keys.append(np.arange(len(pts), len(pts) + len(b)))
            pts += _rel(e, b)
        self.num_landmarks = len(pts)
        # libstdc++'s iteration order of the ground-truth map (Simulator2D.cpp:331-344): D's near landmark gets the key of D's block
        # that comes last in it, so that all 65 arc landmarks stand before it in the in-range list
        order = np.zeros(self.num_landmarks, dtype=np.int32)
        O.lib().orc_landmark_iteration_order(self.num_landmarks, order.ctypes.data_as(O.C.POINTER(O.C.c_int)))
        self.order = order
        dk = set(int(k) for k in self.keys[3])
        last = [int(k) for k in order if int(k) in dk][-1]
        near = int(self.keys[3][-1])
        pts[last], pts[near] = pts[near], pts[last]
        self.near_key_D = last
        self.fixed = np.array(pts)

    def _tuned(self, cfg):
        for k, v in TUNE.items():
            setattr(cfg, k, v)
        return cfg

    def oracle_config(self, safe_distance=SAFE):
        cfg = self._tuned(O.default_config(MAP, num_landmarks=self.num_landmarks))
        cfg.safe_distance = safe_distance
        return cfg

    def make_sims(self):
        ocfg = self.oracle_config()
        return [O.OracleSim(ocfg, e, e, start=tuple(self.starts[e]), fixed_landmarks=self.fixed) for e in range(self.n)]

    def engine_config(self, safe_distance=SAFE):
        from drl_graph_exploration_amd import default_config
        cfg = self._tuned(default_config(MAP, num_landmarks=self.num_landmarks, **CAPS))
        cfg.safe_distance = safe_distance
        return cfg

    def action(self, sim, e, kind):
        if kind == "R":
            return REJECT
        veh = sim.ground_truth()[0]
        cx, cy = CENTRES[e]
        th = HEADING + (math.pi if kind == "t" else 0.0)
        dx, dy = cx - veh[0], cy - veh[1]
        c, s = math.cos(veh[2]), math.sin(veh[2])
        return (c * dx + s * dy, -s * dx + c * dy, O.wrap_theta(th - veh[2]))


@functools.lru_cache(maxsize=None)
def world():
    return World()


@functools.lru_cache(maxsize=None)
def reference():
    """The oracle's run of the world, once: actions [step][env][3], codes [step][env], flag / cleared [step][env] (cleared follows
    from the codes: up after a reset, = not obstacle after a step that moved, unchanged by a rejected one), the ground-truth vehicle
    poses [step][env][3] after each step, and states [step][env]: a clone of every oracle after each step (read only)."""
    w = world()
    sims = w.make_sims()
    acts = np.zeros((N_STEPS, w.n, 3))
    codes = np.zeros((N_STEPS, w.n), dtype=np.int64)
    cleared = np.ones((N_STEPS, w.n), dtype=np.uint8)
    veh = np.zeros((N_STEPS, w.n, 3))
    latch = [True] * w.n
    states = []
    for s in range(N_STEPS):
        for e, sim in enumerate(sims):
            acts[s, e] = w.action(sim, e, SCRIPTS[e][s])
            codes[s, e] = sim.simulate(acts[s, e])
            if codes[s, e] != 1:
                latch[e] = codes[s, e] != 2
            cleared[s, e] = latch[e]
            veh[s, e] = sim.ground_truth()[0]
        states.append([sim.clone() for sim in sims])
    for a in (acts, codes, cleared, veh):
        a.setflags(write=False)
    return dict(actions=acts, codes=codes, flag=(codes == 2).astype(np.uint8), cleared=cleared, veh=veh, states=states)
