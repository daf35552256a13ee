"""TEST INFRASTRUCTURE: the beliefs and candidate plans of the SLAM-OG-Shannon cost (drlgx_slam_og_cost), shared by
tests/test_slam_og_cpu.py (which checks on the CPU that the cases are what they claim to be) and tests/test_gpu_slam_og.py.

One world in a 20 m map (900 cells), hand-checkable in the way of tests/fm2_cases.py: two rings of landmarks of 2.5 m radius, 12 m
apart - no pose of one ring's environment ever sees the other ring - and three environments:

  * environment 0 starts at the centre of the ring of 70 landmarks and is compared straight after the reset (P = 1): more landmarks
    than the 64 lanes that stride them in the blend and than the 4 waves that stride them in the update; a plan of K short actions
    predicts exactly 70 K measurements - 70, 140, 210, and 280 (> 256: refused);
  * environment 1 starts at the centre of the ring of 24, takes three short steps inside it (P = 4, every pose sees the whole ring)
    and has plans of 0, 1 and max_actions = 9 actions (216 measurements), one with a core mask (2 of 4 steps are core poses: 48) and
    one that jumps 12 m away and sees nothing;
  * environment 2 starts out of sight of everything: no landmark, so w1 = alpha / 0.
"""
import math

import numpy as np

import fm2_cases as F
import slam_og_ref
from oracle import oracle as O

MAP = 20
MAX_MEAS = F.MAX_MEAS
LM_RTOL, LM_ATOL = F.SIGMA_RTOL, F.SIGMA_ATOL   # what tests/test_gpu_fm2.py holds the pose blocks to
ALPHA = 0.3                                      # off 0.5, so that swapping the two weights would show
RADIUS = 2.5
RING_SIZES = [70, 24]
CENTRES = np.array([[-6.0317, 0.2718], [5.9683, -0.3183]])
HEADINGS = np.array([0.6234, math.pi / 2 + 0.0234])
BLIND_START = (0.1357, 8.6180, -1.2345)
WALK = [(0.5, 0.0, 0.3)] * 3
SHORT = (0.05, 0.0, 0.01)
JUMP = (0.0, 12.0, 0.0)
CAPS = dict(max_poses=8, max_landmarks=sum(RING_SIZES), max_factors=512, max_actions=9)
N_ENVS = 3


def landmarks():
    out = []
    for c, th, n in zip(CENTRES, HEADINGS, RING_SIZES):
        ang = th + (np.arange(n) + 0.5) * 2 * math.pi / n + 0.011   # off the vehicle's axis: nothing on the +-179.9 degree gate
        out.append(np.stack([c[0] + RADIUS * np.cos(ang), c[1] + RADIUS * np.sin(ang)], axis=1))
    return np.concatenate(out)


def starts():
    return np.concatenate([np.concatenate([CENTRES, HEADINGS[:, None]], axis=1), [BLIND_START]])


SCRIPTS = [[], list(WALK), []]

# name: (environment, plan, core mask or None, predicted measurements)
CASES = {
    "big_K0": (0, [], None, 0),
    "big_K1": (0, [SHORT], None, 70),
    "big_K2": (0, [SHORT] * 2, None, 140),
    "big_K3": (0, [SHORT] * 3, None, 210),
    "walked_K0": (1, [], None, 0),
    "walked_K1": (1, [SHORT], None, 24),
    "walked_K9": (1, [SHORT] * 9, None, 216),
    "walked_core": (1, [SHORT, (0.3, 0.0, 0.2), SHORT, (0.2, 0.0, -0.3)], [0, 1, 0, 1], 48),
    "walked_blind": (1, [JUMP], None, 0),
}
OVERFLOW = (0, [SHORT] * 4, None, 280)
BLIND_ENV = 2


def world():
    fixed = landmarks()
    ocfg = O.default_config(MAP, num_landmarks=len(fixed))
    st = starts()
    sims = [O.OracleSim(ocfg, e, e, start=tuple(st[e]), fixed_landmarks=fixed) for e in range(N_ENVS)]
    for s, script in zip(sims, SCRIPTS):
        for act in script:
            s.simulate(act)
    return F.World("slam_og", sims, st, SCRIPTS, fixed, len(fixed), CAPS, {k: v[:2] for k, v in CASES.items()})


def make_engine(w):
    """The engine of the world, reset and stepped beside its oracles (fm2_cases.make_engine on the 20 m map)."""
    import torch
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    n = len(w.sims)
    cfg = default_config(MAP, num_landmarks=w.num_landmarks, **w.caps)
    eng = Engine(cfg, n, 0)
    eng.set_fixed_landmarks(w.fixed)
    eng.reset(np.arange(n), np.arange(n), starts=w.starts)
    for s in range(max(len(sc) for sc in w.scripts)):
        odom = np.array([sc[s] if s < len(sc) else (0.0, 0.0, 0.0) for sc in w.scripts], dtype=np.float64)
        active = np.array([1 if s < len(sc) else 0 for sc in w.scripts], dtype=np.uint8)
        eng.step(torch.tensor(odom, device=eng.device), torch.tensor(active, device=eng.device))
    assert eng.status() == 0
    return eng, cfg


def reference(w, case, alpha=ALPHA, distance=None):
    e, plan, core, _ = CASES[case] if isinstance(case, str) else case
    return slam_og_ref.slam_og_cost(w.sims[e], plan, alpha, core=core, distance=distance)


def sqrt_det_sum_tol(blocks, rtol=LM_RTOL):
    """How far sum_l sqrt(det B_l) can move when every element of every block moves by rtol of itself: d det <= 2 rtol (xx yy + xy^2),
    d sqrt(det) = d det / (2 sqrt(det))."""
    t = 0.0
    for b in np.asarray(blocks).reshape(-1, 2, 2):
        det = b[0, 0] * b[1, 1] - b[0, 1] * b[1, 0]
        t += rtol * (b[0, 0] * b[1, 1] + b[0, 1] * b[1, 0]) / math.sqrt(det)
    return t
