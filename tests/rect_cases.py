"""TEST INFRASTRUCTURE: rectangular, off-centre worlds and the 8-cell window, shared by tests/test_rect_cpu.py (which checks on the
CPU that the cases are what the GPU tests need: shapes, occupancy of the ragged tiles, no knife edge, probes that tell the x
bounds from the y bounds, margins of the restatements) and tests/test_gpu_rect.py.

Every other world of the suite is a square map centred on the origin: rows == cols and map_min_x == map_min_y there.  Here

  * "wide":   vehicle box x in [-9, 5], y in [-2, 4]; map box (20 m padding kept) x in [-29, 25], y in [-22, 24]: 27 columns x 23
              rows at resolution 2 - four distinct bounds, neither extent a multiple of the 8-cell tile (27 = 3 * 8 + 3, 23 = 2 * 8 + 7);
  * "tall":   its transpose: 23 columns x 27 rows;
  * "sector": "wide" with a +-75 degree sensor - the bounding-box sweep is live and its clamps act on unequal extents;
  * "win8":   "wide" with max_range = 7: the candidate-cell window is 8 cells wide, the limit of the map kernel's 8 x 8 slot grid,
              and an open disc of radius 3.5 cells holds up to 41 cell centres - more than the compact stage's 40 per pose.
"""
import math

import numpy as np

import og_cases
from oracle import oracle as O

N_ENVS = 3
NUM_LANDMARKS = 20   # 84 m^2 of vehicle box: landmarks are seen from the start
MAX_POSES = 32
MAX_ACTIONS = og_cases.MAX_ACTIONS
PAD = 20.0           # read_map_params(ext=20): count_explored and the frontier's interior box mean what they mean in the reference
BOXES = {"wide": (-9.0, 5.0, -2.0, 4.0), "tall": (-2.0, 4.0, -9.0, 5.0)}  # vehicle box: min_x, max_x, min_y, max_y
WORLDS = {
    "wide": dict(box="wide", fov_deg=None, max_range=None),
    "tall": dict(box="tall", fov_deg=None, max_range=None),
    "sector": dict(box="wide", fov_deg=75.0, max_range=None),
    "win8": dict(box="wide", fov_deg=None, max_range=7.0),
}
TRANSPOSE = {"wide": "tall", "tall": "wide"}
SHAPES = {"wide": (23, 27), "tall": (27, 23), "sector": (23, 27), "win8": (23, 27)}  # (rows, cols)

RESET = [(1, 1, math.pi / 2)] * 4  # ExplorationEnv.reset (exploration_env.py:389-422)
# 24 actions: the reset, twelve forward moves (env 0 runs into the far corner of the grid, env 1 into the opposite one), a turn in
# place, partial moves, turns
SCRIPT = RESET + [(2, 0, 0)] * 12 + [(0, 0, 2.9), (1.3, 0, 0), (0, 0, -1.1), (2, 0, 0), (2, 0, 0), (0.4, 0, 0.5), (1.5, 0, 0),
                                     (0.7, 0, -0.4)]
# three turns in place at the start (every pose of the short trajectory stands on the start's spot), then moves; no reset loop
SCRIPT_WIN8 = [(0, 0, 0.8), (0, 0, -1.7), (0, 0, 2.3), (2, 0, 0), (1.3, 0, 0), (0, 0, 0.9), (2, 0, 0), (0.6, 0, 0.3)]
# off-lattice start poses.  wide / sector: env 0 heads for the corner (max_x, max_y), env 1 for (min_x, min_y), env 2 stays around
STARTS = {
    "wide": np.array([[4.8183, 3.7282, 0.7854], [-7.4142, -0.8971, -2.3453], [-1.1357, 1.6180, -1.2345]]),
    "tall": np.array([[2.7282, 3.3183, 0.8174], [-0.8971, -7.4142, -2.3671], [-0.6180, -7.6357, 0.3345]]),
    # cell centres of "wide" lie at even x and odd y.  Env 0: 0.56 m (0.28 cell) off the centre (-2, 1) along y, env 2: as far
    # off the centre (2, 3) along x - two of the spots whose disc of radius 3.5 cells holds 41 centres; env 1: a generic spot
    "win8": np.array([[-2.0, 1.56, 0.3123], [1.1357, 1.6180, -1.2345], [2.56, 3.0, 2.0453]]),
}
STARTS["sector"] = STARTS["wide"]
# boundary probes, one per side of the map box: (start pose, one odometry increment).  SS2D.simulate (pyss2d.py:173-176) tests the
# INCREMENT against the map box, x against the x bounds and y against the y bounds: each probe's verdict flips when the bounds
# of the two axes are exchanged.  The accepted ones keep the vehicle inside the map box.
PROBES = {
    "wide": [((-8.3183, 1.2718, 0.1234), (24.5, 0.0, 0.0)),    # max_x = 25: in  (max_y = 24: out)
             ((0.4142, 1.1029, 0.2453), (0.0, 24.5, 0.0)),     # max_y = 24: out (max_x = 25: in)
             ((4.1357, 2.2180, -0.1345), (-25.0, 0.0, 0.0)),   # min_x = -29: in  (min_y = -22: out)
             ((-3.2183, 0.7282, 0.3234), (0.0, -25.0, 0.0))],  # min_y = -22: out (min_x = -29: in)
    "tall": [((1.2718, -8.3183, 0.1234), (24.5, 0.0, 0.0)),    # max_x = 24: out
             ((1.2718, -8.3183, 0.1234), (0.0, 24.5, 0.0)),    # max_y = 25: in
             ((0.7282, 4.1357, 0.2234), (-25.0, 0.0, 0.0)),    # min_x = -22: out
             ((0.7282, 4.1357, 0.2234), (0.0, -25.0, 0.0))],   # min_y = -29: in
}
# pose chunks: "wide", two envs driven to 66 poses by a loop that stays in the vehicle box (test_gpu_rect: max_poses = 72)
CHUNK_STARTS = np.array([[-6.3183, -0.2718, 0.1234], [2.1357, 2.0180, 3.1153]])
CHUNK_LOOP = [(2, 0, 0)] * 3 + [(0, 0, math.pi / 2)] + [(1.2, 0, 0)] + [(0, 0, math.pi / 2)]
CHUNK_STEPS = 66
CHUNK_CHECKS = (62, 63, 65)  # script indices after which P = 64, 65 and 67


def _apply(c, name):
    spec = WORLDS[name]
    x0, x1, y0, y1 = BOXES[spec["box"]]
    c.env_min_x, c.env_max_x, c.env_min_y, c.env_max_y = x0, x1, y0, y1
    c.map_min_x, c.map_max_x, c.map_min_y, c.map_max_y = x0 - PAD, x1 + PAD, y0 - PAD, y1 + PAD
    c.resolution = 2.0
    if spec["fov_deg"] is not None:
        c.min_bearing, c.max_bearing = -math.radians(spec["fov_deg"]), math.radians(spec["fov_deg"])
    if spec["max_range"] is not None:
        c.max_range = spec["max_range"]
    return c


def oracle_config(name):
    return _apply(O.default_config(14, num_landmarks=NUM_LANDMARKS), name)


def engine_config(name, max_poses=MAX_POSES):
    from drl_graph_exploration_amd import default_config
    # (every pose can sight every landmark of so small a box: the factor table is sized for that)
    return _apply(default_config(14, num_landmarks=NUM_LANDMARKS, max_poses=max_poses, max_actions=MAX_ACTIONS,
                                 max_factors=NUM_LANDMARKS * max_poses), name)


def script_of(name):
    return SCRIPT_WIN8 if name == "win8" else SCRIPT


def fresh_sims(name, cfg_name=None):
    """The world's three oracle instances at their start poses (cfg_name: another world's configuration under the same starts)."""
    ocfg = oracle_config(cfg_name or name)
    return [O.OracleSim(ocfg, i, i, start=tuple(STARTS[name][i])) for i in range(N_ENVS)]


def make_sims(name):
    sims = fresh_sims(name)
    for act in script_of(name):
        for s in sims:
            s.simulate(act)
    return sims


def make_envs(name):
    """OracleEnv per instance (its constructor runs the reset's four actions); the caller steps SCRIPT[4:]."""
    return [O.OracleEnv(14, i, num_landmarks=NUM_LANDMARKS, start=tuple(STARTS[name][i]), cfg=oracle_config(name)) for i in range(N_ENVS)]


def plans_for(sim):
    """og_cases.plans_for without its pose counts around 64: K = 0, 1, the spiral of max_actions, and a straight run out of the map
    box (og_cases sizes its own by map_max_x alone; here by the diagonal, which leaves either rectangle along any heading)."""
    p = og_cases.plans_for(sim)
    c = sim.cfg
    leave = [(0.0, 0.0, 0.3)] + [(2.0, 0.0, 0.0)] * int(math.ceil(math.hypot(c.map_max_x - c.map_min_x, c.map_max_y - c.map_min_y) / 2.0))
    return [p[0], p[1], p[2], leave]


def em_plans_for(sim):
    """The same for the expected look-ahead cost, whose argument check refuses more than 256 predicted measurements: the spiral would be
    cut to the longest prefix that predicts at most 256.  From the beliefs after SCRIPT nothing is cut - every env stands 10 m or more
    from the vehicle box by then - and tests/test_rect_cpu.py asserts the full max_actions, so that a changed world cannot shorten
    the plan unnoticed."""
    from oracle import fm2_ref
    plans = plans_for(sim)
    n_meas = fm2_ref.fm2_update(sim, plans[2])[1]
    keep = int(np.searchsorted(np.cumsum(n_meas), 256, side="right"))
    plans[2] = plans[2][:keep]
    return plans


class OgView(object):
    """One world under the names tests/test_gpu_og.py's Ctx reads from og_cases."""

    def __init__(self, world):
        self.N_ENVS, self.MAX_ACTIONS, self.SCRIPT, self.STARTS = N_ENVS, MAX_ACTIONS, script_of(world), STARTS[world]
        self.engine_config, self.make_sims, self.plans_for = engine_config, make_sims, plans_for


def window(cfg):
    return int(math.ceil(2.0 * cfg.max_range / cfg.resolution)) + 1


def window_origin(cfg, x, y):
    """(row, col) of the first cell of the candidate window of a pose at (x, y), as the map kernel places it."""
    return (int(math.floor((y - cfg.max_range - cfg.map_min_y) / cfg.resolution - 0.5)),
            int(math.floor((x - cfg.max_range - cfg.map_min_x) / cfg.resolution - 0.5)))


def cell_of(cfg, x, y):
    return int(math.floor((y - cfg.map_min_y) / cfg.resolution)), int(math.floor((x - cfg.map_min_x) / cfg.resolution))


def in_range_cells(sim):
    """Per pose of the estimated trajectory: the cell centres of the grid nearer than max_range."""
    cfg = sim.cfg
    rows, cols = sim.vm_shape()
    X, Y = np.meshgrid(cfg.map_min_x + cfg.resolution * (np.arange(cols) + 0.5), cfg.map_min_y + cfg.resolution * (np.arange(rows) + 0.5))
    return [int(np.sum(np.sqrt((X - x) ** 2 + (Y - y) ** 2) < cfg.max_range)) for x, y, _ in sim.poses()[0]]


def accepts(cfg, odom, swapped=False):
    """The bounds predicate of SS2D.simulate on an odometry increment; swapped: x tested against the y bounds and y against x's."""
    bx, by = (cfg.map_min_x, cfg.map_max_x), (cfg.map_min_y, cfg.map_max_y)
    if swapped:
        bx, by = by, bx
    return bx[0] < odom[0] < bx[1] and by[0] < odom[1] < by[1]


# tree sampler: em_plan trees of 65 accepted nodes (one past a wave of lanes) and rrt goals far across each grid, from the belief
# after the script, with em_tree_cases' Halton start indices and node capacity
TREE_NODES = 65
RRT_GOALS = {"wide": np.array([[-20.3, 10.7], [18.4, -14.2], [-12.6, 17.3]]), "tall": np.array([[-14.2, 18.4], [17.3, -12.6], [10.7, -20.3]])}
