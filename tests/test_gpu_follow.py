"""GPU tests (run with -m gpu on an MI355X) of drlgx_follow_plans (k_follow_select / k_follow_record, csrc/k_misc.hip) against its
restatement in tests/follow_ref.py: the same actions one Engine.step at a time with the flags read after each.  Compared: the
stop codes, counts and done flags exactly, the trace rows bit for bit (the record's metrics are drlgx_metrics' bits), the beliefs
bit for bit.  Plans and results are hand-made tensors; no tree is involved."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import follow_ref as R  # noqa: E402
from follow_ref import FWD, JAG, JIG, REJECT  # noqa: E402

# (start, result, active, plan, pre-steps, expected (n_exec, stop)) per env; steps = 3, max_steps = 4 (an env with two steps behind
# it is done behind its second action)
MIX1 = [("far", R.SUCCESS, 1, [JIG, JAG], 0, (2, R.RAN)),                         # plan shorter than steps
        ("far", R.SUCCESS, 1, [JIG, JAG, JIG], 0, (3, R.RAN)),                    # ... equal
        ("far", R.SUCCESS, 1, [JIG, JAG, JIG, JAG, JIG], 0, (3, R.RAN)),          # ... longer
        ("far", R.SAMPLING_FAILURE, 1, [JIG, JAG], 0, (1, R.RAN)),                # the fallback move
        ("far", R.NO_SOLUTION, 1, [JIG, JAG, JIG], 0, (0, R.STOP_NO_SOLUTION)),
        ("far", R.TERMINATION, 1, [JIG, JAG, JIG], 0, (0, R.STOP_TERMINATION)),
        ("far", R.SUCCESS, 0, [JIG, JAG, JIG], 0, (0, R.RAN)),                    # inactive
        ("near", R.SUCCESS, 1, [JIG, JAG, JIG], 0, (1, R.OBSTACLE))]              # obstacle at action 0
MIX2 = [("far", R.SUCCESS, 1, [FWD, FWD, JIG], 0, (2, R.OBSTACLE)),               # obstacle in the middle
        ("far", R.SUCCESS, 1, [JIG, FWD, FWD], 0, (3, R.OBSTACLE)),               # ... at the last action
        ("far", R.SUCCESS, 1, [REJECT, JIG, JAG], 0, (0, R.REJECTED)),            # rejected odometry at action 0
        ("far", R.SUCCESS, 1, [JIG, REJECT, JAG], 0, (1, R.REJECTED)),            # ... in the middle
        ("far", R.SUCCESS, 1, [JIG, JAG, JIG], 2, (2, R.DONE)),                   # done in the middle (step > max_steps)
        ("near", R.SAMPLING_FAILURE, 1, [], 0, (1, R.OBSTACLE)),                  # the fallback turn beside the landmark
        ("far", R.TERMINATION, 0, [JIG], 0, (0, R.STOP_TERMINATION)),             # inactive, and its result says why
        ("near", R.SUCCESS, 1, [JIG, JAG, JIG, JAG], 2, (1, R.OBSTACLE))]         # (the latch is up again after two pre-steps)
STEPS0 = [(s, r, a, p, k, ((1 if r == R.SAMPLING_FAILURE and a else 0),
                           {R.NO_SOLUTION: R.STOP_NO_SOLUTION, R.TERMINATION: R.STOP_TERMINATION}.get(r, R.RAN)))
          for s, r, a, p, k, _ in MIX1[:7]] + [MIX1[6]]
# without the obstacle opt-in the call never stops for an obstacle (the last env then runs into `done` behind its second action)
PLAIN = [m[:5] + (want,) for m, want in zip(MIX2, [(3, R.RAN), (3, R.RAN), (0, R.REJECTED), (1, R.REJECTED), (2, R.DONE), (1, R.RAN),
                                                    (0, R.STOP_TERMINATION), (2, R.DONE)])]
CASES = {"mix1": (MIX1, 3, True), "mix2": (MIX2, 3, True), "steps0": (STEPS0, 0, True), "no_opt_in": (PLAIN, 3, False)}


def _engine(mix, obstacles):
    from drl_graph_exploration_amd.engine import Engine
    eng = Engine(R.engine_config(), R.N, 0)
    eng.set_fixed_landmarks(R.fixed_landmarks())
    eng.reset(np.arange(R.N), np.arange(R.N), starts=R.starts([m[0] for m in mix]))
    if obstacles:
        eng.set_env_obstacles(True)
    pre = max(m[4] for m in mix)
    for k in range(pre):  # pre-steps of some envs: two jiggles (near K: flagged, then held - the latch is up again behind them)
        mask = torch.tensor([1 if m[4] > k else 0 for m in mix], dtype=torch.uint8, device=eng.device)
        eng.step(torch.tensor([JIG if k % 2 == 0 else JAG] * R.N, dtype=torch.float64, device=eng.device), mask)
    assert eng.status() == 0
    return eng


def _dump(eng, i):
    return eng.poses(i) + eng.landmarks(i) + eng.factors(i) + eng.ground_truth(i) + eng.virtual_map(i)


@pytest.mark.parametrize("name", list(CASES))
def test_follow_plans_equals_stepwise(name):
    mix, steps, obstacles = CASES[name]
    plans, results, active = [m[3] for m in mix], [m[1] for m in mix], [m[2] for m in mix]
    dev, ref = _engine(mix, obstacles), _engine(mix, obstacles)
    plan, n_act, res, act = R.tensors(dev, plans, results, active)
    trace, n_exec, done, stop = dev.follow_plans(plan, n_act, res, steps=steps, active=act, max_steps=4)
    trace, n_exec, done, stop = dev.fetch(trace, n_exec, done, stop)
    rows, r_exec, r_done, r_stop = R.follow_stepwise(ref, plans, results, active, steps, max_steps=4)
    print("%s: n_exec %s stop %s done %s (stepwise %s %s %s)" % (name, list(n_exec), list(stop), list(done), r_exec, r_stop, r_done))
    assert list(n_exec) == r_exec and list(stop) == r_stop and list(done) == r_done
    assert [(int(n), int(s)) for n, s in zip(n_exec, stop)] == [m[5] for m in mix]  # ... and the case is what it is listed as
    for e in range(R.N):
        got = trace[e, :n_exec[e]]
        want = np.array(rows[e], dtype=np.float64).reshape(-1, 4)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg="trace rows of env %d" % e)
        assert np.isnan(trace[e, n_exec[e]:]).all()
        assert dev.counts(e) == ref.counts(e)
        for x, y in zip(_dump(dev, e), _dump(ref, e)):
            np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg="env %d" % e)
    fd, fr = dev.obstacle_flags(), ref.obstacle_flags()
    assert torch.equal(fd[0], fr[0]) and torch.equal(fd[1], fr[1])
    assert dev.status() == 0 and ref.status() == 0
    dev.close()
    ref.close()
