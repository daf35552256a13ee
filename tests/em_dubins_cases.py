"""TEST INFRASTRUCTURE: the cases that the CPU and GPU tests of the tree sampler's Dubins control model share: four beliefs on the
12 m box after the script of tests/em_tree_cases.py, four libraries around the 64-entry stride of the library scan, and the goals
and Halton start indices found by a search with tests/em_dubins_ref.py over the CPU oracle's beliefs.  tests/test_em_dubins_cpu.py
asserts the conditions on the oracle's beliefs, tests/test_gpu_em_dubins.py again on the engine's own.

A library has nv x nw x 2 x nd entries - velocities, rates, the two signs, durations - so its size is always EVEN: no parameters give
65 entries.  The library just above the stride has 66."""
import numpy as np

import em_dubins_ref as D
import em_tree_cases as K
from oracle import oracle as O

N_ENVS = 4
SEEDS = [0, 1, 2, 3]
STARTS = np.array([K.STARTS[0], K.STARTS[1], K.STARTS[2], [0.5772, -1.2020, 0.9159]])
CAP = 128
MAX_ACTIONS = 40
MARGIN = 1e-9    # nearest-node (relative), tolerance-radius, safety and isReached margins demanded of every case compared exactly

#                 max_w  dw    min_v max_v dv    dt   min_d max_d tolerance
LIB_36 = D.Params(0.5,  0.25, 0.5,  1.0,  0.25, 0.5, 1.0,  2.0,  0.6)   # 3 velocities x 3 rates x 2 signs x 2 durations
LIB_64 = D.Params(0.75, 0.25, 0.25, 1.0,  0.25, 0.5, 1.0,  2.0,  0.6)   # 4 x 4 x 2 x 2
LIB_66 = D.Params(0.5,  0.05, 0.5,  1.0,  0.25, 0.5, 1.5,  2.0,  0.6)   # 3 x 11 x 2 x 1
LIB_320 = D.Params(0.7, 0.1,  0.6,  1.0,  0.1,  0.5, 1.0,  3.0,  0.6)   # 5 x 8 x 2 x 4: one velocity fills one stride of 64
LIBS = {"36": LIB_36, "64": LIB_64, "66": LIB_66, "320": LIB_320}
SIZES = {"36": 36, "64": 64, "66": 66, "320": 320}
# scripts/envs/pyplanner2d.ini's [Dubins] section: 51 x 51 x 2 x 15
LIB_SHIPPED = D.Params(0.5, 0.01, 0.5, 1.0, 0.01, 0.2, 1.0, 4.0, 0.3)
SHIPPED_SIZE = 78030
# a library nothing connects to: every connect is refused, the counter of 1000 ends the tree
LIB_TIGHT = D.Params(0.5, 0.25, 0.5, 1.0, 0.25, 0.5, 1.0, 2.0, 1e-4)

SAFE_DISTANCE = 1.5

START_INDICES = [0, K.START_INDICES[1], 99999, 31337]
# goals per (library, environment) at safe_distance 0.  Found: every tree but the two marked reaches its goal with 9 .. 123 accepted
# nodes, hundreds to thousands of refused connects, every margin above 1e-6; the 320-entry trees win with entries 0, 63, 64 and 319
# and have accepted connects with further matches in the winner's stride and in later strides (the 36- and 64-entry ones in the one
# stride there is)
GOALS = {
    "36": [(3.79, 5.98), (0.67, 7.58), (3.96, -4.81), (-1.51, 7.08)],    # (env 3: found no goal that is reached)
    "64": [(1.67, -2.91), (-1.9, -2.88), (-1.02, 3.16), (-1.51, 7.08)],
    "66": [(-0.15, 6.9), (-5.52, 6.85), (4.49, -3.85), (-1.51, 7.08)],   # (env 3: as above)
    "320": [(1.24, 5.24), (-3.6, 7.05), (-1.87, 0.2), (7.52, 1.42)],
}
# goals whose goal edge finds no library path (320 entries): SUCCESS, the goal not in the tree, an empty plan
REFUSED_GOALS = [(2.39, 7.03), (-6.8, 2.85), (6.41, -0.93), (-2.5, -5.92)]
# under the obstacle opt-in at SAFE_DISTANCE, 320 entries: (env, goal, start index).  Found: the first four refuse 18 / 2 / 3 / 9
# connects for an unsafe intermediate pose and accept paths whose first or last pose is unsafe (not tested: 0+3 / 1+0 / 1+2 / 0+1);
# the last two reach their goals
OBSTACLE_CASES = [(0, (-2.46, 6.07), 25824), (1, (-3.72, -2.2), 87795), (2, (0.89, -3.42), 64136), (3, (-3.65, -2.42), 32569),
                  (1, (-5.79, -2.18), K.START_INDICES[1]), (3, (7.36, 0.95), 31337)]

# for the facades (their engines have max_actions = 22; both environments from the facade's default Halton index, 320 entries):
# goals reached in 14 and 16 steps, margins above 1e-5
FACADE_GOALS = [(5.58, 2.55), (-2.57, -2.33)]

_libs = {}


def library(name):
    if name not in _libs:
        _libs[name] = D.Library(LIBS[name] if isinstance(name, str) else name)
    return _libs[name]


def make_sims():
    ocfg = O.default_config(K.MAP, num_landmarks=K.NUM_LANDMARKS)
    sims = [O.OracleSim(ocfg, s, s, start=tuple(STARTS[i])) for i, s in enumerate(SEEDS)]
    for act in K.SCRIPT:
        for s in sims:
            s.simulate(act)
    return sims


def tree_of(cfg, root_xytheta, lib, start, goal, keys=(), landmarks=(), safe_distance=0.0, cap=CAP):
    return D.grow(tuple(root_xytheta), K.bounds(cfg), cfg.angle_weight, cfg.max_edge_length, start, cap, lib, tuple(goal), keys,
                  landmarks, safe_distance)


def entitled(t):
    """Whether a tree's decisions all have the margins that exact comparisons need."""
    return min(t.margin, default=1.0) > MARGIN and t.stats.gate_margin > MARGIN and t.stats.match_margin > MARGIN
