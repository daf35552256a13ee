"""TEST INFRASTRUCTURE: the cases that the CPU and GPU tests of the tree sampler's obstacle logic share.  Two sets of beliefs:
  A  the three beliefs of tests/em_tree_cases.py (every nearest landmark's key is below the number of landmarks);
  B  four beliefs with ONE FIXED LANDMARK (key 0) placed where belief 0's pose estimate ends - 0.036 m from it, so that the shrink
     reaches optimize2's clamp to 0 and rrt_planner's non-terminating case - and three more (seed, start) pairs: two whose nearest
     landmark has a key that is NOT below the number of landmarks (no shrink, whatever the distance), one ordinary.
The safe distances, goals and start indices below were found by a search with tests/em_safe_ref.py over the CPU oracle's beliefs;
the margins the search found are noted beside them, and tests/test_em_safe_cpu.py asserts them again on the oracle's beliefs,
tests/test_gpu_em_safe.py on the engine's own."""
import numpy as np

import em_safe_ref as S
import em_tree_cases as K
from oracle import oracle as O

CAP = 128
MARGIN = 1e-9            # gate and step margins demanded of every case compared exactly
N_ACCEPT = 100           # accepted nodes of the trees under obstacles
# set A at 1.5 (a value pyplanner2d.ini ships; at 1.0 and 2.0 the waypoint l = max_edge_length meets d = max_edge_length to the
# last bit - a step margin of 0 - which no exact comparison survives).  Found: rejected samples 2 / 1 / 1, rejected edges 16 / 5 / 8,
# accepted edges with 2 waypoints in all three, gate margins 7.6e-4 / 6.0e-2 / 1.1e-2, step margins 3.8e-2 / 1.8e-2 / 8.4e-2
SAFE_DISTANCE = 1.5
# rrt goals of set A whose goal edge is unsafe at 1.5 (gate margins 7.6e-4 / 8.0e-2 / 1.1e-2)
UNSAFE_GOALS = np.array([[5.1000, 6.2253], [-2.2568, 6.0154], [7.5711, -0.1742]])

# set B
FIXED = [(1.068, 1.075)]
B_SEEDS = [0, 19, 11, 1]
B_STARTS = np.array([K.STARTS[0], K.STARTS[1], K.STARTS[2], K.STARTS[2]])
B_NEAR, B_KEY_HIGH, B_WALLED, B_PLAIN = 0, 1, 2, 3
B_START_INDEX = 7
B_ACCEPT = 40
SHRINK_DISTANCE = 3.0    # NEAR: 0.036 m from key 0 -> 0 (optimize2) / -0.064 (rrt_planner); KEY_HIGH: 2.60 m from key 7 of 5 landmarks: kept
B_RRT_GOALS = np.array([[4.38, -3.06], [-7.0, -3.0], [9.7, 6.6], [9.7, 6.6]])
FAIL_DISTANCE = 60.0     # no point of the 52 m box is 60 m from a landmark: KEY_HIGH (not shrunk) cannot sample; PLAIN shrinks to 1.27
WALLED_DISTANCE = 3.9    # WALLED (0.13 m from key 6 of 5 landmarks, not shrunk): every edge from the root is refused (gate margin 1.2e-3)


def make_sims_b():
    ocfg = O.default_config(K.MAP, num_landmarks=K.NUM_LANDMARKS)
    sims = [O.OracleSim(ocfg, s, s, start=tuple(B_STARTS[i]), fixed_landmarks=FIXED) for i, s in enumerate(B_SEEDS)]
    for act in K.SCRIPT:
        for s in sims:
            s.simulate(act)
    return sims


def tree_of(cfg, root_xytheta, keys, landmarks, safe_distance, start, n_accept=None, goal=None, cap=CAP, point_safe=S.point_is_safe):
    return S.grow(tuple(root_xytheta), K.bounds(cfg), cfg.angle_weight, cfg.max_edge_length, start, cap, keys, landmarks, safe_distance,
                  n_accept=n_accept, goal=goal, point_safe=point_safe)


def entitled(t):
    """Whether a tree's decisions all have the margins that exact comparisons need."""
    return min(t.margin, default=1.0) > K.MARGIN and t.stats.gate_margin > MARGIN and t.stats.step_margin > MARGIN
