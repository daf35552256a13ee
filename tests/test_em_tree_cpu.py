"""CPU tests of tests/em_tree_ref.py - the restatement the GPU tests of the tree sampler (tests/test_gpu_em_tree.py) are judged
against - by hand values, and of the margin that entitles those tests to exact parent indices."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import em_tree_cases as K
import em_tree_ref as R
from drl_graph_exploration_amd import planner2d


def test_halton_hand_values():
    assert R.halton(0) == (0.0, 0.0, 0.0)
    assert R.halton(1) == (1.0 / 2, 1.0 / 3, 1.0 / 5)
    h = R.halton(6)  # 6 = 110 (2) = 20 (3) = 11 (5)
    assert h[0] == 3.0 / 8
    assert h[1] == pytest.approx(2.0 / 9, rel=1e-15) and h[2] == pytest.approx(6.0 / 25, rel=1e-15)
    # 99 999 by its digits: the radical inverse mirrors them behind the point
    for base, got in zip((2, 3, 5), R.halton(99999)):
        digits, n = [], 99999
        while n:
            digits.append(n % base)
            n //= base
        want = sum(d * float(base) ** -(k + 1) for k, d in enumerate(digits))
        assert got == pytest.approx(want, rel=1e-14) and 0.0 < got < 1.0
    assert R.halton(99999)[0] == int(format(99999, "b")[::-1], 2) / 2.0 ** 17  # (base 2 is exact)


def test_mt19937_check_value():
    g = R.MT19937(5489)
    for _ in range(9999):
        g.next_u32()
    assert g.next_u32() == 4123659995


def test_start_index_against_the_host_compilers_mt19937(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "start.cpp"
    src.write_text("#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <random>\n"
                   "int main(int c, char **v) {\n  std::mt19937 g(std::strtoul(v[1], 0, 10));\n"
                   "  std::uniform_real_distribution<> u(0.0, 1.0);\n  int n = (int)std::floor((100000 + 1.0 - 0.0) * u(g) + 0.0);\n"
                   "  std::printf(\"%d\\n\", n >= 0 ? (n <= 100000 ? n : 100000) : 0);\n  return 0;\n}\n")
    exe = tmp_path / "start"
    subprocess.check_call([cxx, "-O1", "-std=c++11", "-o", str(exe), str(src)])
    for seed in (K.DEFAULT_SEED, 1, 5489, 123456789):
        want = int(subprocess.check_output([str(exe), str(seed)]).decode())
        assert R.start_index(seed) == want
        assert planner2d.halton_start_index(seed) == want  # (the facade's own restatement)
    assert 0 <= K.START_INDICES[1] <= 100000


def test_hand_tree_of_three_samples():
    """Root (0, 0, 0), map box [0, 8] x [0, 9], angle_weight 0.4, max_edge_length 2, Halton points 1, 2, 3 = (4, 3), (2, 6), (6, 1):
    sample 1 hangs on the root; for sample 2 node 1 at (1.6, 1.2) is nearer (23.31 against 40.25), for sample 3 too (19.48 against
    37.00 and 22.7 from node 2)."""
    t = R.grow((0.0, 0.0, 0.0), (0.0, 8.0, 0.0, 9.0), 0.4, 2.0, 1, 16, n_accept=3)
    assert t.parent == [-1, 0, 1, 1] and t.depth == [0, 1, 2, 2] and t.leaves() == [2, 3] and t.halton_next == 4
    a1 = math.atan2(3.0, 4.0)
    np.testing.assert_allclose(t.xytheta()[1], [1.6, 1.2, a1], atol=1e-15)
    np.testing.assert_allclose(t.action[1], [1.6, 1.2, a1], atol=1e-15)
    assert t.distance[1] == pytest.approx(math.sqrt(4.0 + (0.4 * math.pi) ** 2), rel=1e-14)  # (the parent lies straight behind)
    # sample 2 from node 1: world direction (0.4, 4.8) / |.|, relative bearing = its angle minus node 1's heading
    n2 = math.hypot(0.4, 4.8)
    b2 = math.atan2(4.8, 0.4) - a1
    np.testing.assert_allclose(t.xytheta()[2], [1.6 + 2 * 0.4 / n2, 1.2 + 2 * 4.8 / n2, math.atan2(4.8, 0.4)], atol=1e-14)
    np.testing.assert_allclose(t.action[2], [2 * math.cos(b2), 2 * math.sin(b2), b2], atol=1e-14)
    b3 = math.atan2(-0.2, 4.4) - a1
    np.testing.assert_allclose(t.action[3], [2 * math.cos(b3), 2 * math.sin(b3), b3], atol=1e-14)
    assert t.distance[3] == pytest.approx(t.distance[1] + math.sqrt(4.0 + (0.4 * math.pi) ** 2), rel=1e-14)
    assert t.actions_to(3) == [t.action[1], t.action[3]]
    # the margins of the three decisions: one node; 23.31 / 40.25; 19.48 / 22.7
    assert t.margin[0] == float("inf") and t.margin[1] == pytest.approx(40.2496 / 23.3140 - 1, abs=2e-3)
    # a short edge is not stretched, and the rrt rule connects the goal to the node that reached it
    g = R.grow((0.0, 0.0, 0.0), (0.0, 8.0, 0.0, 9.0), 0.4, 2.0, 1, 16, goal=(2.5, 2.5))
    assert g.parent == [-1, 0, 1] and g.goal_node == 2 and g.result == R.SUCCESS and g.halton_next == 2
    np.testing.assert_allclose(g.xytheta()[2][:2], [2.5, 2.5], atol=1e-15)
    assert R.grow((0.0, 0.0, 0.0), (0.0, 8.0, 0.0, 9.0), 0.4, 2.0, 1, 2, goal=(7.5, 8.5)).result == R.SAMPLING_FAILURE


def test_pick_and_leaves():
    assert R.pick([3.0, 2.0, 2.0, 5.0]) == 1
    assert R.pick([float("nan"), 1.0]) == 0 and R.pick([2.0, float("nan"), 1.0]) == 2 and R.pick([7.0]) == 0
    assert R.Tree(R.make_pose(0, 0, 0)).leaves() == [0]
    assert R.max_nodes_of([0.1, 0.5, 0.39, 0.4], 0.4, 0.75) == 1


def test_every_nearest_node_decision_of_the_gpu_cases_has_a_margin():
    """Over all draws of the largest tree of every (belief, start index) - the smaller trees are its prefixes - and of the rrt
    trees, the gap between the best and the second-best nearest-node distance exceeds 1e-9 relative; no tree is deeper than the
    test engine's max_actions."""
    sims = K.make_sims()
    worst = float("inf")
    for i, sim in enumerate(sims):
        root = sim.poses()[0][-1]
        known = int(np.count_nonzero(sim.virtual_map()[0] < sim.cfg.occupancy_threshold))
        assert known >= 1
        assert R.max_nodes_of(sim.virtual_map()[0], sim.cfg.occupancy_threshold, K.max_nodes_for(known, 0)) == 0
        for start in K.START_INDICES:
            t = K.tree_of(sim.cfg, root, start, n_accept=max(K.NODE_COUNTS))
            assert len(t) == max(K.NODE_COUNTS) + 1 and max(t.depth) <= K.MAX_ACTIONS
            worst = min(worst, min(t.margin))
        g = K.tree_of(sim.cfg, root, K.START_INDICES[i], goal=tuple(K.RRT_GOALS[i]))
        assert g.result == R.SUCCESS and 3 < len(g) < K.CAP and g.depth[g.goal_node] <= K.MAX_ACTIONS
        worst = min(worst, min(g.margin))
    print("smallest nearest-node margin: %.3e" % worst)
    assert worst > K.MARGIN
