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
# the four sides of SS2D.simulate's bounds test (pyss2d.py:173-176): an increment EXACTLY on a bound is outside (the comparison is
# strict) - the bounds are the engine's config's - and one far beyond each; at action 0 it is k_follow_select's test, behind action 0
# k_follow_record's
_CFG = R.engine_config()
ON_XMAX, ON_XMIN = (_CFG.map_max_x, 0.0, 0.0), (_CFG.map_min_x, 0.0, 0.0)
ON_YMAX, ON_YMIN = (0.0, _CFG.map_max_y, 0.0), (0.0, _CFG.map_min_y, 0.0)
OUT_XMIN, OUT_YMAX, OUT_YMIN = (-100.0, 0.0, 0.0), (0.0, 100.0, 0.0), (0.0, -100.0, 0.0)
SIDES = [("far", R.SUCCESS, 1, [JIG, ON_XMAX, JAG], 0, (1, R.REJECTED)),           # on a bound, seen by the record behind action 0
         ("far", R.SUCCESS, 1, [JIG, ON_XMIN, JAG], 0, (1, R.REJECTED)),
         ("far", R.SUCCESS, 1, [JIG, ON_YMAX, JAG], 0, (1, R.REJECTED)),
         ("far", R.SUCCESS, 1, [JIG, ON_YMIN, JAG], 0, (1, R.REJECTED)),
         ("far", R.SUCCESS, 1, [OUT_XMIN, JIG], 0, (0, R.REJECTED)),               # beyond the other three sides, at action 0 ...
         ("far", R.SUCCESS, 1, [JIG, OUT_YMAX, JAG], 0, (1, R.REJECTED)),          # ... and in the middle
         ("far", R.SUCCESS, 1, [OUT_YMIN, JIG], 0, (0, R.REJECTED)),
         ("far", R.SUCCESS, 1, [JIG, JAG, REJECT], 0, (2, R.REJECTED))]            # a rejection at the last action
# max_steps = 4: an env with four steps behind it is done behind its FIRST action
EDGES = [("far", R.SUCCESS, 1, [ON_XMAX, JIG], 0, (0, R.REJECTED)),                # on a bound at action 0: the selection's test
         ("far", R.SUCCESS, 1, [ON_XMIN, JIG], 0, (0, R.REJECTED)),
         ("far", R.SUCCESS, 1, [ON_YMAX, JIG], 0, (0, R.REJECTED)),
         ("far", R.SUCCESS, 1, [ON_YMIN, JIG], 0, (0, R.REJECTED)),
         ("far", R.SUCCESS, 1, [], 0, (0, R.RAN)),                                 # SUCCESS with an empty plan
         ("far", R.SUCCESS, 1, [JIG, JAG, JIG], 4, (1, R.DONE)),                   # done at action 0
         ("near", R.SUCCESS, 1, [JIG, JAG, JIG], 4, (1, R.DONE)),                  # done AND a raised flag at action 0: done wins
         ("far", R.SUCCESS, 1, [JIG, OUT_XMIN], 0, (1, R.REJECTED))]               # a rejection at the plan's last action
# steps at and beyond max_actions (max_steps = 100: nobody is done); a plan of exactly max_actions rows
LONG = [("far", R.SUCCESS, 1, [JIG, JAG] * 3, 0, (R.A_MAX, R.RAN)),                # a plan of exactly A_MAX rows
        ("far", R.SUCCESS, 1, [JIG, JAG, JIG], 0, (3, R.RAN)),
        ("far", R.SUCCESS, 1, [JIG, JAG] * 2 + [JIG, REJECT], 0, (R.A_MAX - 1, R.REJECTED)),   # ... whose last row is rejected
        ("far", R.SAMPLING_FAILURE, 1, [JIG, JAG], 0, (1, R.RAN)),
        ("far", R.SUCCESS, 1, [FWD, FWD, JIG, JAG, JIG, JAG], 0, (2, R.OBSTACLE)),
        ("far", R.SUCCESS, 0, [JIG, JAG] * 3, 0, (0, R.RAN)),
        ("far", R.NO_SOLUTION, 1, [JIG, JAG] * 3, 0, (0, R.STOP_NO_SOLUTION)),
        ("near", R.SUCCESS, 1, [JAG, JIG] * 3, 0, (1, R.OBSTACLE))]
assert len(LONG[0][3]) == R.A_MAX
FLAGGED = {"edges": [6]}  # envs whose last executed step must have raised the obstacle flag, whatever their stop code says
# (mix, steps, obstacle opt-in[, max_steps = 4])
CASES = {"mix1": (MIX1, 3, True), "mix2": (MIX2, 3, True), "steps0": (STEPS0, 0, True), "no_opt_in": (PLAIN, 3, False),
         "sides": (SIDES, 3, True), "edges": (EDGES, 3, True), "steps_a_max": (LONG, R.A_MAX, True, 100),
         "steps_beyond_a_max": (LONG, R.A_MAX + 3, True, 100)}


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
    mix, steps, obstacles, max_steps = (CASES[name] + (4,))[:4]
    plans, results, active = [m[3] for m in mix], [m[1] for m in mix], [m[2] for m in mix]
    dev, ref = _engine(mix, obstacles), _engine(mix, obstacles)
    plan, n_act, res, act = R.tensors(dev, plans, results, active)
    trace, n_exec, done, stop = dev.follow_plans(plan, n_act, res, steps=steps, active=act, max_steps=max_steps)
    trace, n_exec, done, stop = dev.fetch(trace, n_exec, done, stop)
    rows, r_exec, r_done, r_stop = R.follow_stepwise(ref, plans, results, active, steps, max_steps=max_steps)
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
    for e in FLAGGED.get(name, []):
        assert int(fd[0][e]) == 1
    assert dev.status() == 0 and ref.status() == 0
    dev.close()
    ref.close()


def test_the_bounds_are_the_configs_and_strict():
    """What the cases above claim about their increments, against follow_ref.in_box."""
    cfg = R.engine_config()
    for a in (ON_XMAX, ON_XMIN, ON_YMAX, ON_YMIN, OUT_XMIN, OUT_YMAX, OUT_YMIN, REJECT):
        assert not R.in_box(cfg, a)
    for a, i in ((ON_XMAX, 0), (ON_XMIN, 0), (ON_YMAX, 1), (ON_YMIN, 1)):
        inside = list(a)
        inside[i] = float(np.nextafter(a[i], 0.0))
        assert R.in_box(cfg, inside)
    assert (ON_XMAX[0], ON_XMIN[0], ON_YMAX[1], ON_YMIN[1]) == (cfg.map_max_x, cfg.map_min_x, cfg.map_max_y, cfg.map_min_y)


def test_negative_steps_are_refused_and_nothing_runs():
    """steps = -1: drlgx_follow_plans returns DRLGX_E_INVALID before any launch - flags, counts and beliefs are those of a twin that
    was never called."""
    from drl_graph_exploration_amd._lib import DrlgxError
    mix = MIX1
    plans, results, active = [m[3] for m in mix], [m[1] for m in mix], [m[2] for m in mix]
    dev, ref = _engine(mix, True), _engine(mix, True)
    plan, n_act, res, act = R.tensors(dev, plans, results, active)
    with pytest.raises(DrlgxError, match="drlgx error -1"):  # DRLGX_E_INVALID
        dev.follow_plans(plan, n_act, res, steps=-1, active=act, max_steps=4)
    for e in range(R.N):
        assert dev.counts(e) == ref.counts(e)
        for x, y in zip(_dump(dev, e), _dump(ref, e)):
            np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg="env %d" % e)
    fd, fr = dev.obstacle_flags(), ref.obstacle_flags()
    assert torch.equal(fd[0], fr[0]) and torch.equal(fd[1], fr[1])
    assert dev.status() == 0 and ref.status() == 0
    dev.close()
    ref.close()
