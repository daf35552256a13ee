"""TEST INFRASTRUCTURE: the beliefs, Halton start indices and tree sizes that the CPU and GPU tests of the tree sampler share
(tests/test_em_tree_cpu.py checks on the CPU that every nearest-node decision of them has a margin before
tests/test_gpu_em_tree.py demands exact parent indices)."""
import math

import numpy as np

import em_tree_ref as R
from oracle import oracle as O

MAP = 12            # the vehicle's box; the map the sampler draws from is padded to 52 m: 26 x 26 cells
N_ENVS = 3
NUM_LANDMARKS = 8
MAX_POSES = 16
MAX_ACTIONS = 40    # deeper than any tree below (checked on the CPU)
CAP = 300           # node capacity of the topology cases
SCRIPT = [(1, 1, math.pi / 2)] * 4 + [(0, 0, 0.7), (1.5, 0, 0)]
STARTS = np.array([[0.3183, -0.2718, 0.1234], [-1.4142, 0.8971, 2.0453], [1.1357, 1.6180, -1.2345]])
DEFAULT_SEED = 0    # EMPlannerParameter.seed as the ini file ships it
# one start index per environment: 0, the facade's default, the last but one the constructor can draw
START_INDICES = [0, R.start_index(DEFAULT_SEED), 99999]
# accepted nodes where the lane loops wrap (the tree holds one more: the root)
NODE_COUNTS = [0, 1, 63, 64, 65, 257]
MARGIN = 1e-9
# rrt goals: a frontier point per environment, far enough for a tree of some depth
RRT_GOALS = np.array([[4.38, -3.06], [-6.2, 8.4], [9.7, 6.6]])


def make_sims():
    ocfg = O.default_config(MAP, num_landmarks=NUM_LANDMARKS)
    sims = [O.OracleSim(ocfg, i, i, start=tuple(STARTS[i])) for i in range(N_ENVS)]
    for act in SCRIPT:
        for s in sims:
            s.simulate(act)
    return sims


def bounds(cfg):
    return (cfg.map_min_x, cfg.map_max_x, cfg.map_min_y, cfg.map_max_y)


def max_nodes_for(known, n):
    """A max_nodes parameter with floor(known * max_nodes) = n."""
    m = (n + 0.5) / known
    assert int(math.floor(known * m)) == n
    return m


def tree_of(cfg, root_xytheta, start, n_accept=None, goal=None, cap=CAP):
    return R.grow(tuple(root_xytheta), bounds(cfg), cfg.angle_weight, cfg.max_edge_length, start, cap, n_accept=n_accept, goal=goal)
