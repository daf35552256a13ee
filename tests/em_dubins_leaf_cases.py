"""TEST INFRASTRUCTURE: the cases that tests/test_em_dubins_leaf_cpu.py (which asserts on the CPU oracle that they are what they
claim to be) and tests/test_gpu_em_dubins_leaf.py (which runs them on the device) share.

  * STEPS world: the RINGS of tests/fm2_cases.py - environment e starts at the centre of ring e, every landmark of a ring passes
    the sensor gates from anywhere near its centre; environments 1 .. 5 have driven 12 m out and their plans back up into the ring
    in one long action - with engines of max_actions = 32.  A step inside a ring predicts (ring size) measurements, so a non-core
    step there changes the answer by many times the tolerance when the mask is ignored, and the masked count is
    (core steps inside the ring) x (ring size).
  * TREE cases: the four beliefs of tests/em_dubins_cases.py, its libraries of 36 / 64 / 320 entries, optimize2's stop rule."""
import numpy as np

import em_dubins_cases as DC
import em_tree_cases as K
import em_tree_ref as R
import fm2_cases as F

MAX_ACTIONS = 32
CAPS = dict(max_poses=8, max_landmarks=65, max_factors=512, max_actions=MAX_ACTIONS)
BACK, SHORT, BLIND = F.RING_BACK, F.RING_SHORT, (0.5, 0.0, 0.2)


def _mask(k, ones):
    m = [0] * k
    for i in ones:
        m[i] = 1
    return m


# {name: (environment, plan, core)}; the masked counts are in NM (asserted on the CPU)
STEP_CASES = {
    "K1": (1, [BACK], [1]),
    "one_edge": (1, [BACK] + [SHORT] * 3, _mask(4, [3])),                                 # mask 0001
    "two_edges": (1, [BACK] + [SHORT] * 4, _mask(5, [1, 4])),                             # a core step in the middle
    "blind_core": (1, [BLIND, BACK], _mask(2, [0])),                                      # the core pose sees nothing: nm = 0
    "trailing": (1, [BACK, SHORT, SHORT], _mask(3, [0])),                                 # trailing non-core steps
    "fresh_edge": (0, [SHORT] * 4, _mask(4, [3])),                                        # P = 1
    "ring33": (2, [BACK] + [SHORT] * 2, _mask(3, [2])),                                   # 33 landmarks: the lane loops wrap
    "K_max": (1, [BACK] + [SHORT] * (MAX_ACTIONS - 1), _mask(MAX_ACTIONS, [7, 15, 23, 31])),   # 1024 unmasked, 128 masked: served
}
NM = {"K1": 32, "one_edge": 32, "two_edges": 64, "blind_core": 0, "trailing": 32, "fresh_edge": 32, "ring33": 33, "K_max": 128}
# its twin: nine core steps, 288 masked measurements - refused
OVER = (1, [BACK] + [SHORT] * (MAX_ACTIONS - 1), _mask(MAX_ACTIONS, [3, 7, 11, 15, 19, 23, 27, 30, 31]))
COST_CASES = ["one_edge", "two_edges", "blind_core", "trailing", "K_max"]  # handed to em_cost against the numpy reference
TREE_DISTANCE = 7.25  # a distance that is not the plan's own


def steps_world():
    fixed = F.ring_landmarks()
    w = F.rings_world()
    return F.World("steps", w.sims, w.starts, w.scripts, fixed, len(fixed), CAPS, {})


def layout(cases, max_actions=MAX_ACTIONS):
    """(cand_env i32 [C], actions f64 [C, A, 3], n_actions i32 [C], core u8 [C, A]) of a list of (env, plan, core)."""
    c = len(cases)
    env = np.array([e for e, _, _ in cases], dtype=np.int32)
    acts = np.zeros((c, max_actions, 3))
    n = np.zeros(c, dtype=np.int32)
    core = np.zeros((c, max_actions), dtype=np.uint8)
    for i, (_, plan, m) in enumerate(cases):
        n[i] = len(plan)
        acts[i, :len(plan)] = np.array(plan).reshape(-1, 3)
        core[i, :len(m)] = m
    return env, acts, n, core


# ---- trees: (library, safe_distance) with the Halton starts of em_dubins_cases; floor(known * TREE_MAX_NODES) is 6 or 7 accepted
# nodes on these beliefs (29 .. 34 known cells).  Found on the CPU oracle: "36" at 0 ends environment 3 with SAMPLING_FAILURE (1001
# connects without a path from the root), "320" at 1.5 ends environment 2 so (its root's samples are unsafe); the others succeed
# with 2 .. 4 leaves of 6 .. 23 steps
TREE_MAX_NODES = 6.5 / 29
TREE_CAP = 64
TREE_CASES = [("36", 0.0), ("64", 0.0), ("320", 0.0), ("320", DC.SAFE_DISTANCE)]


def tree_of(cfg, root_xytheta, prob, lib, start, keys, landmarks, safe_distance, max_nodes=TREE_MAX_NODES, cap=TREE_CAP):
    import em_dubins_leaf_ref as LR
    n = R.max_nodes_of(prob, cfg.occupancy_threshold, max_nodes)
    return LR.grow(tuple(root_xytheta), K.bounds(cfg), cfg.angle_weight, start, cap, lib, n, keys, landmarks, safe_distance)
