"""TEST INFRASTRUCTURE: the maps, beliefs and candidate plans that the CPU and GPU tests of the expected map entropy share
(tests/test_og_cpu.py checks on the CPU that none of them sits on a knife edge before tests/test_gpu_og.py uses them).

The maps are the smallest at which the kernel can go wrong, so their grids are NOT padded by the 20 m of read_map_params:
  * "small":  a 12 x 12 m map at resolution 2 - 36 cells, less than one wave, one partial 8 x 8 tile - inside a 20 x 20 m vehicle
              box: ground-truth landmarks fall outside the grid and every sector sweep is clamped;
  * "mid":    the 40 x 40 m map - 400 cells, 20 is no multiple of 8;
  * "sector": "small" with a +-75 degree sensor: the sweep's bounding box prunes (it is provably no restriction for the full
              circle, where the kernel skips it) and the field of view is decided by the exact bearing.
"""
import math

import numpy as np

from oracle import oracle as O

CONFIGS = {
    "small": dict(env=20, map_half=6.0, num_landmarks=14, fov_deg=None),
    "mid": dict(env=40, map_half=20.0, num_landmarks=40, fov_deg=None),
    "sector": dict(env=20, map_half=6.0, num_landmarks=14, fov_deg=75.0),
}
N_ENVS = 3
MAX_POSES = 16
MAX_ACTIONS = 64
SCRIPT = [(1, 1, math.pi / 2)] * 4 + [(0, 0, 0.7), (1.5, 0, 0)]  # P = 7: old poses, landmarks and re-sightings all exist
STARTS = np.array([[0.3183, -0.2718, 0.1234], [-1.4142, 0.8971, 2.0453], [1.1357, 1.6180, -1.2345]])


def _apply(c, spec):
    h = spec["map_half"]
    c.map_min_x, c.map_max_x, c.map_min_y, c.map_max_y = -h, h, -h, h
    if spec["fov_deg"] is not None:
        c.min_bearing, c.max_bearing = -math.radians(spec["fov_deg"]), math.radians(spec["fov_deg"])
    return c


def oracle_config(name):
    spec = CONFIGS[name]
    return _apply(O.default_config(spec["env"], num_landmarks=spec["num_landmarks"]), spec)


def engine_config(name):
    from drl_graph_exploration_amd import default_config
    spec = CONFIGS[name]
    return _apply(default_config(spec["env"], num_landmarks=spec["num_landmarks"], max_poses=MAX_POSES, max_actions=MAX_ACTIONS), spec)


def make_sims(name):
    ocfg = oracle_config(name)
    sims = [O.OracleSim(ocfg, i, i, start=tuple(STARTS[i])) for i in range(N_ENVS)]
    for act in SCRIPT:
        for s in sims:
            s.simulate(act)
    return sims


def plans_for(sim):
    """The parity cases of one environment: K = 0, 1 and max_actions; P + K = 63, 64, 65; a straight run out of the map box."""
    P = sim.num_poses()
    assert P + MAX_ACTIONS >= 65 > P
    spiral = [(0.0, 0.0, 0.4)] + [(0.23, 0.0, 0.117)] * (MAX_ACTIONS - 1)
    wrap = [[(0.31, 0.0, 0.091 + 0.005 * d)] * (63 + d - P) for d in range(3)]
    leave = [(0.0, 0.0, 0.3)] + [(2.0, 0.0, 0.0)] * int(math.ceil((sim.cfg.map_max_x + 8.0) / 2.0))
    return [[], [(0.0, 0.0, 1.3)], spiral] + wrap + [leave]


def leaves_the_map(sim, plan):
    import em_ref
    p = em_ref.leaf_poses(sim, plan)[-1]
    c = sim.cfg
    return not (c.map_min_x <= p[0] < c.map_max_x and c.map_min_y <= p[1] < c.map_max_y)


def landmarks_outside_the_grid(sim):
    c = sim.cfg
    xy = sim.landmarks()[1]
    return int(np.sum((xy[:, 0] < c.map_min_x) | (xy[:, 0] >= c.map_max_x) | (xy[:, 1] < c.map_min_y) | (xy[:, 1] >= c.map_max_y)))
