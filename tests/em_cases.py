"""TEST INFRASTRUCTURE: the belief and the candidate plans that the CPU and GPU tests of the expected look-ahead cost share
(tests/test_em_cpu.py checks on the CPU that none of them sits on a knife edge before tests/test_gpu_em.py uses them)."""
import math

import numpy as np

from oracle import oracle as O

MAP = 40
N_ENVS = 4
NUM_LANDMARKS = 60
# the first 11 actions of the script of tests/test_gpu_belief.py: P = 12, old poses, landmarks and re-sightings all exist
SCRIPT = [(1, 1, math.pi / 2)] * 4 + [(0, 0, 0.7), (2, 0, 0), (2, 0, 0), (1.3, 0, 0), (0, 0, -1.1), (2, 0, 0), (2, 0, 0)]
# the three plans of test_fm2_covariance_update_matches_the_restatement
FM2_PLANS = [[(0.0, 0.0, -0.7), (2.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.8, 0.0, 0.0)], [(0.0, 0.0, 2.4), (2.0, 0.0, 0.0)],
             [(0.0, 0.0, 0.3), (2.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 0.0, 0.0), (1.1, 0.0, 0.0)]]


def generic_starts(n):
    """Start poses off the integer lattice (tests/test_gpu_belief.py): no cell sits exactly on a range / FOV boundary."""
    return np.array([O.start_pose(lo, MAP / 2 + 20) for lo in range(n)]) + np.array([0.3183, -0.2718, 0.1234])


def make_sims(n=N_ENVS):
    ocfg = O.default_config(MAP, num_landmarks=NUM_LANDMARKS)
    starts = generic_starts(n)
    sims = [O.OracleSim(ocfg, lo, lo, start=tuple(starts[lo])) for lo in range(n)]
    for act in SCRIPT:
        for s in sims:
            s.simulate(act)
    return sims, starts


def blind_jump(sim):
    """One action that lands where no estimated landmark is within reach of the sensor: no predicted measurement.  The first
    such offset on a fixed search pattern around the last estimate (body frame), off the cell lattice."""
    cfg = sim.cfg
    xyt, _ = sim.poses()
    x, y, th = xyt[-1]
    _, lm, _ = sim.landmarks()
    for radius in (7.3, 8.9, 10.7, 12.3, 14.1):
        for k in range(16):
            phi = 0.137 + k * math.pi / 8
            dx, dy = radius * math.cos(phi), radius * math.sin(phi)
            nx, ny = x + math.cos(th) * dx - math.sin(th) * dy, y + math.sin(th) * dx + math.cos(th) * dy
            inside = cfg.env_min_x + 1 < nx < cfg.env_max_x - 1 and cfg.env_min_y + 1 < ny < cfg.env_max_y - 1
            if inside and (len(lm) == 0 or np.min(np.hypot(lm[:, 0] - nx, lm[:, 1] - ny)) > cfg.max_range + 0.5):
                return [(dx, dy, 0.21)]
    raise AssertionError("no landmark-free spot on the search pattern")


def plans_for(sim, max_actions):
    """The parity cases of one environment: the three fm2 plans, no action, a pure rotation, a max_actions-long arc, and a jump
    away from every estimated landmark."""
    arc = [(0.0, 0.0, 0.4)] + [(0.6, 0.0, 0.07)] * (max_actions - 1)
    return FM2_PLANS + [[], [(0.0, 0.0, 1.3)], arc, blind_jump(sim)]
