"""GPU tests of the lazy restore (drlgx_restore leaves the virtual-map planes in the snapshot; the next belief step rebuilds them,
any other entry point copies them first): an engine created with DRLGX_RESTORE_EAGER=1 (the full copy) and one created without it
are driven through the same calls and must agree BIT FOR BIT on everything bench.py --dump-outputs writes, plus utility, metrics,
the graph export and the status word."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench  # noqa: E402  (the headline's configuration and warm-up script)


def _engine(n_envs, eager, n_roll=64, max_snapshots=2):
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    cfg = default_config(bench.MAP, num_landmarks=bench.NUM_LM, max_poses=41, max_landmarks=100, max_factors=12 * 41 + 20,
                         max_snapshots=max_snapshots)
    old = os.environ.pop("DRLGX_RESTORE_EAGER", None)
    try:
        if eager:
            os.environ["DRLGX_RESTORE_EAGER"] = "1"
        eng = Engine(cfg, n_envs, n_roll)  # (the switch is read once, when the engine is created)
    finally:
        os.environ.pop("DRLGX_RESTORE_EAGER", None)
        if old is not None:
            os.environ["DRLGX_RESTORE_EAGER"] = old
    ids = np.arange(n_envs)
    eng.reset(ids, ids, los=ids)
    for act in bench.WARM_SCRIPT:
        eng.step(torch.tensor([act] * n_envs, dtype=torch.float64, device=eng.device))
    eng.check_status()
    eng.snapshot(0)
    return eng


def _odom(eng, act=bench.STEP_ACTION):
    return torch.tensor([act] * eng.n_envs, dtype=torch.float64, device=eng.device)


def _diverge(eng):
    """Move every env one step away from snapshot 0 (another action than the headline's), so that its virtual-map planes and its
    covariance panel differ from the snapshot's: a restore that leaves them behind cannot pass unnoticed."""
    eng.restore(0)
    eng.step(_odom(eng, (0.0, 0.0, 0.9)))


def _state(eng, tmp, tag):
    """Everything a caller can read back: bench.py's output dump, utility, metrics, the graph export, the status word."""
    d = os.path.join(str(tmp), tag)
    bench.dump_outputs(eng, d)
    out = {k[:-4]: np.load(os.path.join(d, k)) for k in sorted(os.listdir(d))}
    out["utility_fresh"] = eng.utility().cpu().numpy()
    out["metrics_fresh"] = eng.metrics().cpu().numpy()
    g = eng.graph()
    for k in ("x", "edge_index", "edge_attr", "node_off", "edge_off", "n_frontier", "frontier_xy", "nearest_frontier_node"):
        out["graph_" + k] = g[k].cpu().numpy()
    out["status"] = np.array([eng.status()])
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        # bit for bit: compare the bytes (NaNs included)
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)
    assert int(a["status"][0]) == 0, what


@pytest.fixture(scope="module")
def pair():
    eager, lazy = _engine(bench.N_ENVS, True), _engine(bench.N_ENVS, False)
    yield eager, lazy
    eager.close()
    lazy.close()


def _both(pair, fn):
    for eng in pair:
        fn(eng)


def test_restore_step_bench_state(pair, tmp_path):
    def run(eng):
        _diverge(eng)
        eng.restore(0)
        eng.step(_odom(eng))
    _both(pair, run)
    _assert_same(_state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l"), "restore + step")


def test_restore_step_inactive_and_rejected(pair, tmp_path):
    n = bench.N_ENVS
    def run(eng):
        active = torch.ones(n, dtype=torch.uint8, device=eng.device)
        active[3::7] = 0
        odom = _odom(eng)
        odom[5::11, 0] = 1000.0  # outside the map box: SS2D.simulate rejects the move
        _diverge(eng)
        eng.restore(0)
        eng.step(odom, active)
    _both(pair, run)
    _assert_same(_state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l"), "restore + masked / rejected step")


@pytest.mark.parametrize("getter", ["utility", "metrics", "cov_array", "graph", "virtual_map", "snapshot_then_dump"])
def test_restore_then_getter(pair, tmp_path, getter):
    res = []
    for eng in pair:
        _diverge(eng)
        eng.restore(0)
        if getter == "virtual_map":
            r = [np.asarray(v) for i in (0, 17, bench.N_ENVS - 1) for v in eng.virtual_map(i)]
        elif getter == "graph":
            r = [eng.graph()["x"].cpu().numpy()]
        elif getter == "cov_array":
            r = [t.cpu().numpy() for t in eng.cov_array()]
        elif getter == "snapshot_then_dump":
            eng.snapshot(1)  # (slot 1 now holds the restored state: restoring it must give the same belief)
            eng.restore(1)
            r = []
        else:
            r = [getattr(eng, getter)().cpu().numpy()]
        res.append(r)
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes(), getter
    _assert_same(_state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l"), "restore + " + getter)


def test_restore_snapshot_step_restore_step(pair, tmp_path):
    def run(eng):
        _diverge(eng)
        eng.restore(0)
        eng.snapshot(1)
        eng.step(_odom(eng))
        eng.restore(1)
        eng.step(_odom(eng, (0.0, 0.0, 0.6)))
    _both(pair, run)
    _assert_same(_state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l"), "restore, snapshot, step, restore, step")


def test_restore_other_slot_then_step(pair, tmp_path):
    def run(eng):
        eng.restore(0)
        eng.step(_odom(eng))
        eng.snapshot(1)  # slot 1: one step further than slot 0
        _diverge(eng)
        eng.restore(0)
        eng.restore(1)
        eng.step(_odom(eng))
    _both(pair, run)
    _assert_same(_state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l"), "restore 0, restore 1, step")
    def run2(eng):
        _diverge(eng)
        eng.restore(1)
        eng.restore(0)
        eng.step(_odom(eng))
    _both(pair, run2)
    _assert_same(_state(pair[0], tmp_path, "e2"), _state(pair[1], tmp_path, "l2"), "restore 1, restore 0, step")


def test_restore_reset_subset_step(pair, tmp_path):
    ids = np.arange(0, bench.N_ENVS, 5)
    def run(eng):
        _diverge(eng)
        eng.restore(0)
        eng.reset(ids, 1000 + ids, los=ids)
        eng.step(_odom(eng, (1.0, 1.0, math.pi / 2)))
    _both(pair, run)
    _assert_same(_state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l"), "restore, reset of a subset, step")


def test_restore_lookahead(pair, tmp_path):
    rewards = []
    env_ids = list(range(0, bench.N_ENVS, 8))
    for eng in pair:
        eng.restore(0)
        ce = torch.tensor(env_ids, dtype=torch.int32, device=eng.device)
        # goals a step or two from each robot: the plans fit the 41 poses of the engine (36 + a few actions)
        goals = []
        for k, i in enumerate(env_ids):
            xyt = eng.poses(i)[0][-1]
            goals.append([xyt[0] + (0.7 if k % 2 else -0.6), xyt[1] + 0.4 * (k % 3 - 1)])
        goals = torch.tensor(goals, dtype=torch.float64, device=eng.device)
        actions, n_act = eng.line_plan(ce, goals)
        _diverge(eng)
        eng.restore(0)  # (the look-ahead comes right behind this restore)
        rewards.append(eng.lookahead(ce, actions, n_act).cpu().numpy())
    assert rewards[0].tobytes() == rewards[1].tobytes()
    _assert_same(_state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l"), "restore + lookahead")


def test_restore_step_staged_kernels(pair, tmp_path):
    _both(pair, lambda eng: (_diverge(eng), eng.restore(0), eng.step(_odom(eng))))
    fused = _state(pair[1], tmp_path, "fused")
    def run(eng):
        _diverge(eng)
        eng.timing_enable(2)
        eng.restore(0)
        eng.step(_odom(eng))
        eng.timing_enable(False)
        eng.timing_read()
    _both(pair, run)
    staged_e, staged_l = _state(pair[0], tmp_path, "e"), _state(pair[1], tmp_path, "l")
    _assert_same(staged_e, staged_l, "restore + staged step")
    _assert_same(fused, staged_l, "staged against fused step")


def test_restore_step_split_map_2048():
    # more envs than CUs: the fused step leaves the map stage out and k_map_c runs behind it (it takes over the restore's debt)
    n = 2048
    a, b = _engine(n, True, n_roll=0, max_snapshots=1), _engine(n, False, n_roll=0, max_snapshots=1)
    try:
        res = []
        for eng in (a, b):
            active = torch.ones(n, dtype=torch.uint8, device=eng.device)
            active[9::13] = 0
            odom = _odom(eng)
            odom[4::17, 0] = 1000.0
            _diverge(eng)
            eng.restore(0)
            eng.step(odom, active)
            r = [eng.utility().cpu().numpy(), eng.metrics().cpu().numpy()] + [t.cpu().numpy() for t in eng.cov_array()]
            r += [np.asarray(v) for i in (0, 4, 9, 1000, n - 1) for v in eng.virtual_map(i)]
            r.append(np.array([eng.status()]))
            res.append(r)
        for k, (x, y) in enumerate(zip(*res)):
            assert x.tobytes() == y.tobytes(), k
        assert int(res[1][-1][0]) == 0
    finally:
        a.close()
        b.close()
