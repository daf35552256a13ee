"""CPU tests of the host layers around drlgx_og_plan (optimize2 under OG_SHANNON / SLAM_OG_SHANNON): the library's export, the
header's declaration, em_baseline's command line, and the facades' routing of the four algorithms, on a stub engine."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry():
    from drl_graph_exploration_amd import _lib
    assert "drlgx_og_plan" in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.lib_path()), "drlgx_og_plan")


def test_header_declares_the_entry_and_the_algorithms():
    text = open(os.path.join(ROOT, "include", "drlgx.h")).read()
    assert re.search(r"^int drlgx_og_plan\(drlgx_engine \*e, int n_sel, const int32_t \*env_sel_dev, const int32_t \*halton_start_dev, "
                     r"int max_tree_nodes,\s+int algorithm, double alpha,", text, re.M)
    assert re.search(r"^#define DRLGX_ALG_OG_SHANNON 2\b", text, re.M) and re.search(r"^#define DRLGX_ALG_SLAM_OG_SHANNON 3\b", text, re.M)


def test_baseline_command_line():
    from drl_graph_exploration_amd import em_baseline
    from drl_graph_exploration_amd.planner2d import EMPlannerParameter
    ap = em_baseline.build_parser()
    for name, alg in (("OG_SHANNON", 2), ("SLAM_OG_SHANNON", 3), ("EM_AOPT", 0), ("EM_DOPT", 1)):
        assert ap.parse_args(["--algorithm", name]).algorithm == name and em_baseline.ALGORITHMS[name] == alg
    assert ap.parse_args([]).alpha == EMPlannerParameter().alpha and ap.parse_args(["--alpha", "0.25"]).alpha == 0.25
    with pytest.raises(SystemExit):
        ap.parse_args(["--algorithm", "SHANNON"])
    assert em_baseline.csv_path("out", 40, "SLAM_OG_SHANNON") == os.path.join("out", "40_EM_SLAM_OG_SHANNON.csv")


class StubEngine(object):
    """Records which planner entry a facade calls."""

    def __init__(self):
        self.calls = []

    def em_plan(self, env_sel, halton_start, max_tree_nodes=1024, algorithm=0, want_nodes=False):
        self.calls.append(("em_plan", int(algorithm), want_nodes))
        return "em"

    def og_plan(self, env_sel, halton_start, max_tree_nodes=1024, algorithm=2, alpha=0.0, want_nodes=False):
        self.calls.append(("og_plan", int(algorithm), float(alpha), want_nodes))
        return "og"


def test_facades_route_the_four_algorithms():
    from drl_graph_exploration_amd import planner2d, pyplanner2d
    from drl_graph_exploration_amd.planner2d import OptimizationAlgorithm as Alg
    prm = planner2d.EMPlannerParameter()
    prm.alpha = 0.25
    eng = StubEngine()
    for alg in Alg:
        prm.algorithm = alg
        planner2d.plan_trees(eng, prm, None, None, 64, want_nodes=True)
    assert eng.calls == [("em_plan", 0, True), ("em_plan", 1, True), ("og_plan", 2, 0.25, True), ("og_plan", 3, 0.25, True)]
    prm.dubins_control_model_enabled = True  # the Dubins control model stays out under the OG algorithms
    with pytest.raises(NotImplementedError):
        planner2d.plan_trees(eng, prm, None, None, 64)
    prm.dubins_control_model_enabled = False

    # EMPlanner2D.optimize2 and EMExplorer's planner hand their engine call to plan_trees with the parameter as it is now
    class Planner(planner2d.EMPlanner2D):
        def __init__(self, parameter):
            self._parameter = parameter

        def _tree_call(self, run, rrt=False):
            return run(eng, None, None)

    class Owner(object):
        _planner_params = prm

    class ExplorerPlanner(pyplanner2d._Planner):
        def __init__(self):
            self._o = Owner()

        def _call(self, run, rrt=False):
            return run(eng, None, None)

    for alg, want in ((Alg.SLAM_OG_SHANNON, ("og_plan", 3, 0.25, True)), (Alg.EM_DOPT, ("em_plan", 1, True))):
        prm.algorithm = alg
        for planner in (Planner(prm), ExplorerPlanner()):
            del eng.calls[:]
            args = (None, None) if isinstance(planner, Planner) else ()
            assert planner.optimize2(*args) == want[0][:2] and eng.calls == [want]
