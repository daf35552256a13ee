"""GPU tests (run with -m gpu on an MI355X) of the EM baseline's episodes under the two occupancy-grid algorithms: em_baseline.run
against a hand-written loop of Engine.og_plan + Engine.follow_plans on a second engine with the same seeds (compared exactly), its
CSV, and EMPlanner2D.optimize2 under OG_SHANNON on the module classes."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS, DECISIONS, STEPS = [0, 1, 2], 2, 5
ALGORITHMS = {"OG_SHANNON": 2, "SLAM_OG_SHANNON": 3}
ALPHA = 0.3   # (off the parameter's default 0.5: a run that ignored it would show)
_records = {}


@pytest.fixture(scope="module")
def records():
    from drl_graph_exploration_amd import em_baseline

    def get(name):
        if name not in _records:
            _records[name] = em_baseline.run(algorithm=name, seeds=SEEDS, max_decisions=DECISIONS, steps=STEPS, alpha=ALPHA)
        return _records[name]
    yield get
    _records.clear()


@pytest.mark.parametrize("name", sorted(ALGORITHMS))
def test_records_equal_a_hand_written_loop(records, name):
    from drl_graph_exploration_amd import em_baseline
    from drl_graph_exploration_amd.planner2d import halton_start_index
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    rec = records(name)
    n = len(SEEDS)
    env = VecExplorationEnv(40, n, env_index=SEEDS, test=True, max_poses=256, n_rollouts=0, algorithm=ALGORITHMS[name], alpha=ALPHA)
    try:
        e = env.engine
        e.set_env_obstacles(True)
        e.set_sampler_parameter(em_baseline.MAX_NODES, em_baseline.PLANNER_SAFE_DISTANCE)
        e.set_sampler_obstacles(True)
        assert [r["seed"] for r in rec] == [int(s) for s in env.env_index]
        sel = torch.arange(n, dtype=torch.int32, device=env.device)
        start = torch.full((n,), halton_start_index(0), dtype=torch.int32, device=env.device)
        live = np.ones(n, dtype=bool)
        rows = 0
        for d in range(DECISIONS):
            o = e.og_plan(sel, start, 2048, ALGORITHMS[name], ALPHA)
            start = o["halton_next"]
            trace, n_exec, done, stop = e.follow_plans(o["plan"], o["n_actions"], o["result"], steps=STEPS,
                                                       active=torch.as_tensor(live.astype(np.uint8), device=env.device), sigma0=1.0,
                                                       done_explored=0.85, max_steps=env._max_steps)
            trace, n_exec, done, stop, plan, n_act, result = e.fetch(trace, n_exec, done, stop, o["plan"], o["n_actions"], o["result"])
            for i in np.nonzero(live)[0]:
                dec = rec[i]["decisions"][d]
                assert dec["result"] == result[i] and dec["stop"] == stop[i] and len(dec["rows"]) == n_exec[i] <= STEPS
                assert dec["plan"] == plan[i, :n_act[i]].tolist()
                assert dec["rows"] == trace[i, :n_exec[i], :3].tolist() and dec["explored"] == trace[i, :n_exec[i], 3].tolist()
                rows += int(n_exec[i])
                live[i] = not (done[i] or stop[i] >= 4)
        assert e.status() == 0 and rows > 0 and all(len(r["decisions"]) <= DECISIONS for r in rec)
    finally:
        env.close()


@pytest.mark.parametrize("name", sorted(ALGORITHMS))
def test_csv_name_and_category(records, name, tmp_path):
    from drl_graph_exploration_amd import em_baseline, evaluate
    path = em_baseline.csv_path(str(tmp_path), 40, name)
    assert path.endswith("40_EM_%s.csv" % name)
    evaluate.write_csv(records(name), path, "EM+" + name, 40)
    lines = open(path).read().splitlines()
    assert lines[0] == evaluate.HEADER and len(lines) > 1 and all(ln.split(",")[0] == "EM+" + name for ln in lines[1:])


def test_optimize2_of_the_module_classes_under_og_shannon():
    from drl_graph_exploration_amd import planner2d, ss2d
    from drl_graph_exploration_amd.pyplanner2d import config_from_ini
    from oracle import oracle as O
    from test_gpu_em_tree import same_odoms
    from test_gpu_modules import MAP, ini
    lo = 3
    start = tuple(np.array(O.start_pose(lo, MAP / 2 + 20)) + np.array([0.2871, -0.3179, 0.0917]))
    cp = ini(lo)
    cp.set("Planner", "algorithm", "OG_SHANNON")
    cp.set("Planner", "safe_distance", "0.0")
    cp.set("Planner", "max_nodes", "0.1")
    _, prm = config_from_ini(cp)
    sim = ss2d.Simulator2D(prm["sensor"], prm["control"], lo)
    sim.initialize_vehicle(ss2d.Pose2(*start))
    slam = ss2d.SLAM2D(prm["map"])
    virtual_map = ss2d.VirtualMap(prm["virtual_map"], lo)
    sim.random_landmarks([], 8, prm["environment"])
    slam.add_prior(ss2d.VehicleBeliefState(sim.vehicle, np.diag([1.0 / 0.05 ** 2, 1.0 / 0.05 ** 2, 1.0 / math.radians(0.01) ** 2])))
    for key, m in sim.measure():
        slam.add_measurement(key, m)
    slam.optimize(update_covariance=True)
    planner = planner2d.EMPlanner2D(prm["planner"], sim.sensor_model, sim.control_model)
    assert int(planner.get_parameter().algorithm) == 2
    for odom in [(1, 1, math.pi / 2)] * 4 + [(2.0, 0.0, 0.0), (0.0, 0.0, 0.8)]:
        _, control_state = sim.move(ss2d.Pose2(*odom), True)
        slam.add_odometry(control_state)
        sim.measure()
        for key, m in sim.measure():
            slam.add_measurement(key, m)
        slam.optimize(update_covariance=True)
        virtual_map.update_probability(slam, sim.sensor_model)
        virtual_map.update_information(slam.map, sim.sensor_model)
    first = planner.halton_next
    assert first == planner2d.halton_start_index(lo)
    assert planner.optimize2(slam, virtual_map) == planner2d.OptimizationResult.SUCCESS
    plan = []
    for edge in planner.iter_solution():
        plan.insert(0, edge.get_odoms()[0])
    e = slam._ses.engine
    o = e.og_plan(torch.zeros(1, dtype=torch.int32, device=e.device), torch.tensor([first], dtype=torch.int32, device=e.device),
                  planner.MAX_TREE_NODES, 2)
    want = o["plan"][0, :int(o["n_actions"][0])].cpu().numpy()
    assert len(plan) == len(want) > 0 and planner.halton_next == int(o["halton_next"][0])
    same_odoms(np.array([[a.x, a.y, a.theta] for a in plan]), want)  # (x, y exactly; theta went through a Pose2: 1e-15)
    e.check_status()
