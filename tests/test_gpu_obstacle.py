"""GPU tests (run with -m gpu on an MI355X) of SS2D.simulate's obstacle flag on the device (drlgx_set_env_obstacles,
ksim::k_sim_step_obs) on the world of tests/obstacle_cases.py, whose transitions tests/test_obstacle_cpu.py proves on the CPU.

The flag and the latch are compared with the oracle's EXACTLY, step by step; the beliefs with the parity bar of DESIGN.md section 2
(compare_state: RNG-path values 1e-12, estimates 1e-9, information rtol 1e-7 / atol 1e-6, virtual map 1e-7); opted-in against plain
runs bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import obstacle_cases as OC  # noqa: E402
from test_gpu_belief import compare_state  # noqa: E402


def _engine(cfg, w, obstacles, eager=None):
    from drl_graph_exploration_amd.engine import Engine
    old = os.environ.pop("DRLGX_RESTORE_EAGER", None)
    try:
        if eager:
            os.environ["DRLGX_RESTORE_EAGER"] = "1"
        eng = Engine(cfg, w.n, 0)
    finally:
        os.environ.pop("DRLGX_RESTORE_EAGER", None)
        if old is not None:
            os.environ["DRLGX_RESTORE_EAGER"] = old
    eng.set_fixed_landmarks(w.fixed)
    eng.reset(np.arange(w.n), np.arange(w.n), starts=w.starts)
    assert eng.status() == 0
    if obstacles:
        eng.set_env_obstacles(True)
    return eng


def _step(eng, acts):
    eng.step(torch.tensor(acts, dtype=torch.float64, device=eng.device))


def _flags(eng):
    f, c = eng.obstacle_flags()
    return f.cpu().numpy(), c.cpu().numpy()


def _dump(eng, i):
    return eng.poses(i) + eng.landmarks(i) + eng.factors(i) + eng.ground_truth(i) + eng.virtual_map(i)


def _assert_bits(a, b, msg):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg=msg)


def test_flags_equal_the_oracle_and_the_beliefs_do_not_change():
    """Opted in: flag and cleared equal the oracle's at every step of every env, the beliefs stay within the parity bar.  The same
    world without the opt-in: all-zero flags, and poses, landmarks, factors, ground truth (the control stream) and virtual map bit
    for bit those of the opted-in engine - at every step, so both random streams sit at the same place throughout."""
    w, ref = OC.world(), OC.reference()
    on, off = _engine(w.engine_config(), w, True), _engine(w.engine_config(), w, False)
    f, c = _flags(on)
    assert not f.any() and c.all()  # pyss2d.py:132
    for s in range(OC.N_STEPS):
        _step(on, ref["actions"][s])
        _step(off, ref["actions"][s])
        f, c = _flags(on)
        print("step %d flag %s cleared %s (oracle %s %s)" % (s, f, c, ref["flag"][s], ref["cleared"][s]))
        np.testing.assert_array_equal(f, ref["flag"][s], err_msg="flag, step %d" % s)
        np.testing.assert_array_equal(c, ref["cleared"][s], err_msg="cleared, step %d" % s)
        f0, c0 = _flags(off)
        assert not f0.any() and c0.all()
        for i in range(w.n):
            compare_state(on, i, ref["states"][s][i], "env %s step %d" % (OC.NAMES[i], s))
            assert on.counts(i) == off.counts(i)
            _assert_bits(_dump(on, i), _dump(off, i), "opt-in on / off, env %s step %d" % (OC.NAMES[i], s))
    assert on.status() == 0 and off.status() == 0
    on.close()
    off.close()


def test_safe_distance_zero_opted_in_is_inert():
    w, ref = OC.world(), OC.reference()
    zero, off = _engine(w.engine_config(safe_distance=0.0), w, True), _engine(w.engine_config(safe_distance=0.0), w, False)
    for s in range(OC.N_STEPS):
        _step(zero, ref["actions"][s])
        _step(off, ref["actions"][s])
        f, c = _flags(zero)
        assert not f.any() and c.all()
    for i in range(w.n):
        assert zero.counts(i) == off.counts(i)
        _assert_bits(_dump(zero, i), _dump(off, i), "safe_distance 0, env %s" % OC.NAMES[i])
    assert zero.status() == 0 and off.status() == 0
    zero.close()
    off.close()


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
def test_snapshot_carries_the_latch(eager):
    """Snapshot after step 0 (A, B, D, E, F have the latch down, C up), steps 1 and 2, restore, steps 1 and 2 again: the same
    flags both times, and the oracle's - a restore that lost the latch would flag A, D and F at step 1.  Lazy: the step directly
    behind the restore takes over the planes; eager: the full copy."""
    w, ref = OC.world(), OC.reference()
    eng = _engine(w.engine_config(), w, True, eager=eager)
    _step(eng, ref["actions"][0])
    assert list(_flags(eng)[1]) == list(ref["cleared"][0]) and not ref["cleared"][0].all() and ref["cleared"][0].any()
    eng.snapshot(0)
    runs = []
    for _ in range(2):
        seen = []
        for s in (1, 2):
            _step(eng, ref["actions"][s])  # (directly behind the restore: no other entry point settles the lazy restore's debt)
            seen.append(_flags(eng))
            np.testing.assert_array_equal(seen[-1][0], ref["flag"][s])
            np.testing.assert_array_equal(seen[-1][1], ref["cleared"][s])
        runs.append((seen, [_dump(eng, i) for i in range(w.n)]))
        eng.restore(0)
    for (fa, ca), (fb, cb) in zip(runs[0][0], runs[1][0]):
        np.testing.assert_array_equal(fa, fb)
        np.testing.assert_array_equal(ca, cb)
    for i in range(w.n):
        _assert_bits(runs[0][1][i], runs[1][1][i], "after the restore, env %s" % OC.NAMES[i])
    _step(eng, ref["actions"][1])  # the restore at the end of the loop: step once more from the snapshot
    np.testing.assert_array_equal(_flags(eng)[0], ref["flag"][1])
    assert eng.status() == 0
    eng.close()
