"""GPU tests (run with -m gpu on an MI355X) of SS2D.simulate's obstacle flag on the device (ksim::k_sim_step_obs, ksim::measure<kObs>,
ksim::scan_in_range) where the in-range list wraps its trips of 64, on the worlds of tests/obstacle_wrap_cases.py, whose claims
tests/test_obstacle_wrap_cpu.py proves on the CPU; and of the forms of the step under the opt-in that tests/test_gpu_obstacle.py
does not run: the pose-chain solver, timing mode 2, an `active` mask, a reset of a subset, a look-ahead between two steps, step_plans.

No tolerance of its own: the flag and the latch are compared with the oracle's EXACTLY, step by step; the beliefs with
test_gpu_belief.compare_state at its bar; opted-in against plain runs (and twins) bit for bit with test_gpu_obstacle's _dump.

Observed on an MI355X (printed by the tests): see DESIGN.md, "EM baseline episodes"."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import obstacle_wrap_cases as WC  # noqa: E402
from test_gpu_belief import compare_state  # noqa: E402
from test_gpu_obstacle import _assert_bits, _dump, _flags, _step  # noqa: E402

WORLDS = {"W": (WC.world_w, WC.reference_w), "A": (WC.world_a, WC.reference_a)}
# the bound of the simulator launches' LDS (include/drlgx.h, cfg.num_landmarks): 64 KB, of which the stream images take 5 008 B (k_reset:
# 7 512 B) and the launch 16 B + 20 B per landmark (the opt-in 36 B, the look-ahead's pre-simulation 24 B)
LDS = 64 * 1024
LG_OBS = (LDS - 5008 - 16) // 36
LG_CREATE = (LDS - 7512 - 16) // 20
LG_CREATE_ROLLOUTS = (LDS - 5008 - 16) // 24


def _engine(w, cfg, obstacles, n_rollouts=0, by_capacity=False):
    from drl_graph_exploration_amd.engine import Engine
    old = os.environ.pop("DRLGX_VARIANT_BY_CAPACITY", None)
    try:
        if by_capacity:
            os.environ["DRLGX_VARIANT_BY_CAPACITY"] = "1"
        eng = Engine(cfg, w.n, n_rollouts)
    finally:
        os.environ.pop("DRLGX_VARIANT_BY_CAPACITY", None)
        if old is not None:
            os.environ["DRLGX_VARIANT_BY_CAPACITY"] = old
    eng.set_fixed_landmarks(w.fixed)
    eng.reset(np.arange(w.n), np.arange(w.n), starts=w.starts)
    assert eng.status() == 0
    if obstacles:
        eng.set_env_obstacles(True)
    return eng


def _check_step(w, ref, s, on, off=None, envs=None, what=""):
    """After step s: `on`'s flag and latch are the oracle's, its beliefs within the parity bar, and bit for bit those of `off`."""
    f, c = _flags(on)
    envs = range(w.n) if envs is None else envs
    print("%sstep %d flag %s cleared %s (oracle %s %s)" % (what, s, f, c, ref["flag"][s], ref["cleared"][s]))
    for i in envs:
        assert f[i] == ref["flag"][s][i] and c[i] == ref["cleared"][s][i], "%senv %s step %d" % (what, w.names[i], s)
        compare_state(on, i, ref["states"][s][i], "%senv %s step %d" % (what, w.names[i], s))
        if off is not None:
            assert on.counts(i) == off.counts(i)
            _assert_bits(_dump(on, i), _dump(off, i), "%sopt-in on / off, env %s step %d" % (what, w.names[i], s))


@pytest.mark.parametrize("name", list(WORLDS))
def test_stepwise_flags_equal_the_oracle_and_the_plain_engine(name):
    w, ref = WORLDS[name][0](), WORLDS[name][1]()
    cfg = w.engine_config(ref["caps"])
    on, off = _engine(w, cfg, True), _engine(w, cfg, False)
    f, c = _flags(on)
    assert not f.any() and c.all()  # pyss2d.py:132
    for s in range(w.n_steps):
        _step(on, ref["actions"][s])
        _step(off, ref["actions"][s])
        _check_step(w, ref, s, on, off, what="world %s " % name)
        f0, c0 = _flags(off)
        assert not f0.any() and c0.all()
    assert on.status() == 0 and off.status() == 0
    on.close()
    off.close()


def test_pose_chain_solver_under_the_opt_in():
    """DRLGX_VARIANT_BY_CAPACITY=1 at max_poses = 43: drlgx_launch_slam picks k_slam_arrow behind k_sim_step_obs."""
    w, ref = WC.world_w(), WC.reference_w()
    cfg = w.engine_config(dict(ref["caps"], max_poses=43))
    on, off = _engine(w, cfg, True, by_capacity=True), _engine(w, cfg, False, by_capacity=True)
    for s in range(3):
        _step(on, ref["actions"][s])
        _step(off, ref["actions"][s])
        _check_step(w, ref, s, on, off, what="pose chain ")
    assert on.status() == 0 and off.status() == 0
    on.close()
    off.close()


def test_timing_mode_2_under_the_opt_in():
    w, ref = WC.world_w(), WC.reference_w()
    cfg = w.engine_config(ref["caps"])
    on, off = _engine(w, cfg, True), _engine(w, cfg, False)
    on.timing_enable(2)
    for s in range(3):
        _step(on, ref["actions"][s])
        _step(off, ref["actions"][s])
        _check_step(w, ref, s, on, off, what="per stage ")
    t = on.timing_read()
    assert t["sim"][1] == 3 and t["slam"][1] == 3 and t["map"][1] == 3 and t["step"][1] == 0
    assert on.status() == 0 and off.status() == 0
    on.close()
    off.close()


def test_an_inactive_env_keeps_flag_latch_and_state():
    """Step 1 with Y masked out: Y - flagged at step 0, latch down - keeps both and its state bit for bit; X and Z follow the oracle."""
    w, ref = WC.world_w(), WC.reference_w()
    Y = 1
    on = _engine(w, w.engine_config(ref["caps"]), True)
    _step(on, ref["actions"][0])
    f0, c0 = _flags(on)
    assert f0[Y] == 1 and c0[Y] == 0
    before, counts = _dump(on, Y), on.counts(Y)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device=on.device)
    on.step(torch.tensor(ref["actions"][1], dtype=torch.float64, device=on.device), mask)
    f, c = _flags(on)
    assert f[Y] == 1 and c[Y] == 0 and on.counts(Y) == counts
    _assert_bits(_dump(on, Y), before, "the inactive env")
    _check_step(w, ref, 1, on, envs=[0, 2], what="mask ")
    assert on.status() == 0
    on.close()


def test_reset_of_a_subset_leaves_the_other_latches():
    """After step 1 X and Y have the latch down, Z up.  X is reset: it reports (0, cleared), Y keeps (1, latch down).  Then X runs
    its step 0 again (the same seed and start: the oracle's step 0) beside step 2 of Y and Z."""
    w, ref = WC.world_w(), WC.reference_w()
    X, Y, Z = range(3)
    on = _engine(w, w.engine_config(ref["caps"]), True)
    for s in range(2):
        _step(on, ref["actions"][s])
    f, c = _flags(on)
    assert list(c) == [0, 0, 1] == list(ref["cleared"][1]) and list(f) == [1, 1, 0]
    on.reset(np.array([X]), np.array([X]), starts=w.starts[[X]])
    f, c = _flags(on)
    assert list(f) == [0, 1, 0] and list(c) == [1, 0, 1]
    acts = np.array([ref["actions"][0][X], ref["actions"][2][Y], ref["actions"][2][Z]])
    _step(on, acts)
    f, c = _flags(on)
    print("after the reset: flag %s cleared %s" % (f, c))
    for i, s in ((X, 0), (Y, 2), (Z, 2)):
        assert f[i] == ref["flag"][s][i] and c[i] == ref["cleared"][s][i], w.names[i]
        compare_state(on, i, ref["states"][s][i], "env %s after the reset of X" % w.names[i])
    assert on.status() == 0
    on.close()


def test_lookahead_between_two_steps_neither_reads_nor_writes_the_flags():
    w, ref = WC.world_w(), WC.reference_w()
    cfg = w.engine_config(ref["caps"])
    on, off = _engine(w, cfg, True, n_rollouts=4), _engine(w, cfg, False, n_rollouts=4)
    _step(on, ref["actions"][0])
    _step(off, ref["actions"][0])
    f0, c0 = _flags(on)
    assert f0.any() and not c0.all()  # (the rollouts' copies carry a raised flag and a latch that is down)
    rewards = []
    for eng in (on, off):
        ce = torch.tensor([0, 1, 2, 1], dtype=torch.int32, device=eng.device)
        actions = torch.zeros(4, cfg.max_actions, 3, dtype=torch.float64, device=eng.device)
        actions[:, 0] = torch.tensor([0.05, 0.0, 0.01], dtype=torch.float64)
        actions[:, 1] = torch.tensor([-0.05, 0.0, -0.01], dtype=torch.float64)
        actions[3, 2] = torch.tensor([0.3, 0.1, 0.2], dtype=torch.float64)
        n_act = torch.tensor([2, 2, 1, 3], dtype=torch.int32, device=eng.device)
        rewards.append(eng.lookahead(ce, actions, n_act).cpu().numpy())
    print("look-ahead rewards, opt-in on %s off %s" % (rewards[0], rewards[1]))
    assert np.isfinite(rewards[0]).all()
    np.testing.assert_array_equal(rewards[0].view(np.uint64), rewards[1].view(np.uint64))
    f1, c1 = _flags(on)
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_array_equal(c1, c0)
    _step(on, ref["actions"][1])
    _step(off, ref["actions"][1])
    _check_step(w, ref, 1, on, off, what="behind the look-ahead ")
    assert on.status() == 0 and off.status() == 0
    on.close()
    off.close()


def test_step_plans_under_the_opt_in_equals_one_step_per_action():
    """drlgx_step_plans under the opt-in (one drlgx_step_plan per action from a_begin = 0) against a twin's Engine.step per action:
    plans of 4, 2 and 4 actions (Z's last one is the rejected odometry)."""
    w, ref = WC.world_w(), WC.reference_w()
    cfg = w.engine_config(ref["caps"])
    A = cfg.max_actions
    n_act = [4, 2, 4]
    dev, twin = _engine(w, cfg, True), _engine(w, cfg, True)
    plan = torch.tensor(np.ascontiguousarray(ref["actions"][:A].transpose(1, 0, 2)), dtype=torch.float64, device=dev.device)
    dev.step_plans(plan, torch.tensor(n_act, dtype=torch.int32, device=dev.device), A, map_last_only=False)
    for a in range(A):
        mask = torch.tensor([1 if a < n else 0 for n in n_act], dtype=torch.uint8, device=twin.device)
        twin.step(torch.tensor(ref["actions"][a], dtype=torch.float64, device=twin.device), mask)
    fd, cd = _flags(dev)
    ft, ct = _flags(twin)
    print("step_plans flag %s cleared %s (stepwise %s %s)" % (fd, cd, ft, ct))
    np.testing.assert_array_equal(fd, ft)
    np.testing.assert_array_equal(cd, ct)
    for i, n in enumerate(n_act):
        s = n - 1
        assert fd[i] == ref["flag"][s][i] and cd[i] == ref["cleared"][s][i]
        assert dev.counts(i) == twin.counts(i)
        _assert_bits(_dump(dev, i), _dump(twin, i), "step_plans / stepwise, env %s" % w.names[i])
    assert dev.status() == 0 and twin.status() == 0
    dev.close()
    twin.close()


# ---- the host check of the simulator launches' LDS (check_config, drlgx_set_env_obstacles); no test launches an oversized kernel ----
def _sparse_world(num_landmarks):
    """One env: K 0.6 m ahead of the centre, every other listed landmark 30 m and more away."""
    far = [(30.0 + 0.5 * (i % 50), -20.0 + 0.5 * (i // 50)) for i in range(num_landmarks - 1)]
    return WC.World("S", ["c"], ["2"], [WC.W_CENTRES[1]], [[WC.K] + far], 0.0)


SMALL = dict(max_poses=4, max_landmarks=8, max_factors=64, max_actions=4)


def test_opt_in_at_the_largest_accepted_count():
    """num_landmarks = 1 680: k_sim_step_obs takes 36 x 1 680 + 5 024 = 65 504 B of LDS.  One opted-in step, the oracle's flag."""
    assert 36 * LG_OBS + 5024 <= LDS < 36 * (LG_OBS + 1) + 5024 and LG_OBS == 1680
    w = _sparse_world(LG_OBS)
    sim = w.make_sims()[0]
    act = w.action(sim, 0, "c")
    code = sim.simulate(act)
    assert code == 2
    eng = _engine(w, w.engine_config(SMALL), True)
    _step(eng, np.array([act]))
    f, c = _flags(eng)
    assert eng.status() == 0 and f[0] == 1 and c[0] == 0
    compare_state(eng, 0, sim, "1680 listed landmarks")
    eng.close()


def test_opt_in_refused_just_above_its_bound():
    from drl_graph_exploration_amd._lib import DrlgxError
    w = _sparse_world(LG_OBS + 1)
    sim = w.make_sims()[0]
    act = w.action(sim, 0, "c")
    sim.simulate(act)
    eng = _engine(w, w.engine_config(SMALL), False)
    with pytest.raises(DrlgxError, match="drlgx error -3") as err:  # DRLGX_E_CAPACITY
        eng.set_env_obstacles(True)
    assert "k_sim_step_obs" in str(err.value) and not eng.env_obstacles
    _step(eng, np.array([act]))  # the opt-in is off: a plain step, no flag
    f, c = _flags(eng)
    assert eng.status() == 0 and f[0] == 0 and c[0] == 1
    compare_state(eng, 0, sim, "1681 listed landmarks, plain")
    eng.close()


def test_create_refuses_a_landmark_count_the_simulator_cannot_serve():
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd._lib import DrlgxError
    from drl_graph_exploration_amd.engine import Engine
    assert LG_CREATE == 2900 and LG_CREATE_ROLLOUTS == 2521
    for lg, n_roll, ok in ((LG_CREATE, 0, True), (LG_CREATE + 1, 0, False), (LG_CREATE_ROLLOUTS, 2, True), (LG_CREATE_ROLLOUTS + 1, 2, False)):
        cfg = default_config(WC.MAP, num_landmarks=lg, **SMALL)
        if ok:
            Engine(cfg, 1, n_roll).close()  # (created only: nothing is launched at the bound itself)
        else:
            with pytest.raises(DrlgxError, match="num_landmarks too large for the LDS of the simulator kernels"):
                Engine(cfg, 1, n_roll)
