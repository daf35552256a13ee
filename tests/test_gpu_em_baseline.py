"""GPU tests (run with -m gpu on an MI355X) of the EM baseline's host layer: em_baseline.run against a hand-composed em_plan +
follow loop, its CSV, pyplanner2d.explore and EMExplorer.follow_path."""
import math
from configparser import ConfigParser

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS, DECISIONS, STEPS = [0, 1, 2], 2, 5


def _ini(env_sd="0.0", planner_sd="1.0", max_nodes=0.1):
    cp = ConfigParser()
    cp.read_dict({
        "Sensor Model": dict(bearing_noise="0.5", range_noise="0.02", min_bearing="-179.9", max_bearing="179.9", min_range="0.1", max_range="6.0"),
        "Control Model": dict(translation_noise="0.1", rotation_noise="0.2"),
        "Environment": dict(min_x="-6", max_x="6", min_y="-6", max_y="6", max_steps="5000", safe_distance=env_sd),
        "Virtual Map": dict(resolution="2.0", sigma0="1.0", num_samples="1"),
        "Simulator": dict(seed="0", lo="0", num="6", sigma_x0="0.05", sigma_y0="0.05", sigma_theta0="0.01"),
        "Planner": dict(seed="0", angle_weight="0.4", distance_weight0="5.0", distance_weight1="2.0", d_weight="0.0", max_edge_length="2.0",
                        max_nodes=repr(max_nodes), occupancy_threshold="0.4", safe_distance=planner_sd, algorithm="EM_AOPT", reg_out="false",
                        dubins_control_model_enabled="false"),
    })
    return cp


@pytest.fixture(scope="module")
def records():
    from drl_graph_exploration_amd import em_baseline
    return em_baseline.run("EM_AOPT", 40, SEEDS, steps=STEPS, max_decisions=DECISIONS)


def test_records_equal_a_hand_composed_loop(records):
    from drl_graph_exploration_amd import em_baseline
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    env = VecExplorationEnv(40, len(SEEDS), env_index=SEEDS, test=True, max_poses=256, n_rollouts=0)
    env.engine.set_env_obstacles(True)
    assert [r["seed"] for r in records] == [int(s) for s in env.env_index]
    live = np.ones(len(SEEDS), dtype=bool)
    for d in range(DECISIONS):
        plan, n_act, result = env.em_plan(em_baseline.MAX_NODES, 2048, safe_distance=em_baseline.PLANNER_SAFE_DISTANCE)
        trace, n_exec, done, stop = env.follow(plan, n_act, result, steps=STEPS, active=torch.as_tensor(live.astype(np.uint8), device=env.device))
        trace, n_exec, done, stop, plan, n_act, result = env.engine.fetch(trace, n_exec, done, stop, plan, n_act, result)
        for i in np.nonzero(live)[0]:
            dec = records[i]["decisions"][d]
            assert dec["result"] == result[i] and dec["stop"] == stop[i] and len(dec["rows"]) == n_exec[i] <= STEPS
            assert dec["plan"] == plan[i, :n_act[i]].tolist()
            assert dec["rows"] == trace[i, :n_exec[i], :3].tolist() and dec["explored"] == trace[i, :n_exec[i], 3].tolist()
            assert dec["time"] > 0
            live[i] = not (done[i] or stop[i] >= 4)
    assert all(len(r["decisions"]) <= DECISIONS for r in records) and sum(len(d["rows"]) for r in records for d in r["decisions"]) > 0
    env.close()


def test_csv_reads_back(records, tmp_path):
    from drl_graph_exploration_amd import em_baseline, evaluate
    path = em_baseline.csv_path(str(tmp_path), 40, "EM_AOPT")
    assert path.endswith("40_EM_EM_AOPT.csv")
    evaluate.write_csv(records, path, "EM+EM_AOPT", 40)
    lines = open(path).read().splitlines()
    assert lines == evaluate.csv_lines(records, "EM+EM_AOPT", 40) and lines[0] == evaluate.HEADER
    rows = [ln.split(",") for ln in lines[1:]]
    assert all(r[0] == "EM+EM_AOPT" for r in rows)
    want = [row for r in records for d in r["decisions"] for row in d["rows"]]
    got = [[float(r[3]), float(r[4]), float(r[5])] for r in rows if r[3]]
    first = [row for d in records[0]["decisions"] for row in d["rows"]]
    assert got[:len(first)] == first and len(got) >= len(want)  # (a finished episode repeats its last row up to the plot's last step)
    assert [float(r[1]) for r in rows if r[1]] == [d["time"] for r in records for d in r["decisions"]]


def test_explore_stops_at_max_distance():
    from drl_graph_exploration_amd import pyplanner2d
    status, t = pyplanner2d.explore(_ini(), max_distance=0.0)
    assert status == "MAX_DISTANCE" and t > 0
    with pytest.raises(NotImplementedError):
        pyplanner2d.explore(_ini(), save_fig=True)
    with pytest.raises(NotImplementedError):
        pyplanner2d.explore(_ini(), save_history=True)


def test_follow_path_stops_where_the_vector_call_stops():
    """One env, its plan followed by EMExplorer.follow_path (one simulate per edge, the flag fetched after each) and by
    Engine.follow_plans on a twin: the same number of executed steps, the same poses bit for bit, True exactly at a stop."""
    from drl_graph_exploration_amd.pyplanner2d import EMExplorer
    a = EMExplorer(_ini(env_sd="1.5"), obstacle_logic=True, env_obstacles=True)
    b = EMExplorer(_ini(env_sd="1.5"), obstacle_logic=True, env_obstacles=True)
    for ex in (a, b):
        for _ in range(4):
            ex.simulate((0, 0, math.pi / 2.0))
        assert ex.plan()
    p0 = a.engine.counts(0)["poses"]
    hit = a.follow_path(5)
    out = b._planner.last
    A = b.engine.cfg.max_actions  # (done_explored = 2: follow_path knows no `done`)
    trace, n_exec, done, stop = b.engine.follow_plans(out["plan"].view(1, A, 3), out["n_actions"], out["result"], steps=5, done_explored=2.0)
    n_exec, stop = b.engine.fetch(n_exec, stop)
    assert a.engine.counts(0)["poses"] - p0 == n_exec[0]
    assert bool(hit) == (stop[0] in (2, 3))
    np.testing.assert_array_equal(a.engine.poses(0)[0], b.engine.poses(0)[0])
    dub = _ini()
    dub.set("Planner", "dubins_control_model_enabled", "true")
    with pytest.raises(NotImplementedError, match="core=False"):
        EMExplorer(dub).follow_path()
