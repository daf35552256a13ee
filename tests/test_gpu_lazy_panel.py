"""GPU tests of the lazy restore's covariance panels (drlgx_restore leaves the body of every valid panel in the snapshot; the
incremental update of the next belief step reads it there and stores into the env, every other path copies it first): an engine
created with DRLGX_RESTORE_EAGER=1 (the full copy) and one created without it are driven through the same calls on the worlds of
tests/lazy_panel_cases.py and must agree BIT FOR BIT - estimates, information blocks, covariance traces, counts, the virtual map,
utility, metrics, status and the panel itself (header and live extent, drlgx_debug_panel_host) - and the snapshot instances must be
byte for byte what they were."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lazy_panel_cases as LP  # noqa: E402


def _engine(world, eager, n_roll=0):
    from drl_graph_exploration_amd.engine import Engine
    old = os.environ.pop("DRLGX_RESTORE_EAGER", None)
    try:
        if eager:
            os.environ["DRLGX_RESTORE_EAGER"] = "1"
        eng = Engine(world.engine_config(max_snapshots=2), world.n, n_roll)  # (the switch is read once, when the engine is created)
    finally:
        os.environ.pop("DRLGX_RESTORE_EAGER", None)
        if old is not None:
            os.environ["DRLGX_RESTORE_EAGER"] = old
    eng.set_fixed_landmarks(world.fixed)
    return eng


class Pair(object):
    """The eager and the lazy engine of one world."""

    def __init__(self, world, n_roll=0):
        self.world, self.engines = world, (_engine(world, True, n_roll), _engine(world, False, n_roll))

    def close(self):
        for eng in self.engines:
            eng.close()

    def start(self, script):
        """Both engines: reset, the open-loop script, snapshot 0.  Returns the snapshot's bytes (per engine)."""
        n = self.world.n
        for eng in self.engines:
            eng.reset(np.arange(n), np.arange(n), starts=self.world.starts)
            for a in LP.actions(script, n):
                eng.step(torch.tensor(a, device=eng.device))
            assert eng.status() == 0
            eng.snapshot(0)
        return [_snapshot_bytes(eng, 0) for eng in self.engines]

    def run(self, fn):
        return [fn(eng) for eng in self.engines]


def _odom(eng, act):
    return torch.tensor(np.array([act] * eng.n_envs, dtype=np.float64), device=eng.device)


def _instance(eng, i, vm=True):
    c = eng.counts(i)
    out = [np.array([c[k] for k in sorted(c)])]
    out += list(eng.poses(i)) + list(eng.landmarks(i)) + list(eng.cov_traces(i))
    if vm:
        out += [np.asarray(v) for v in eng.virtual_map(i)]
    meta, body = eng.panel(i)
    out.append(meta)
    if body is not None:
        out.append(body)
    return out


def _state(eng):
    out = [eng.utility().cpu().numpy(), eng.metrics().cpu().numpy(), np.array([eng.status()])]
    for i in range(eng.n_envs):
        out += _instance(eng, i)
    return out


def _snapshot_bytes(eng, slot):
    return [x.tobytes() for e in range(eng.n_envs) for x in _instance(eng, eng.snapshot_instance(slot, e))]


def _assert_same(pair, what, snaps=None):
    a, b = pair.run(_state)
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: item %d differs" % (what, k)
    assert int(a[2][0]) == 0, what
    if snaps is not None:  # the snapshot is read-only
        for eng, before in zip(pair.engines, snaps):
            assert _snapshot_bytes(eng, 0) == before, what + ": snapshot 0 changed"


def _diverge(eng):
    """One other step away from snapshot 0: the env's panel and planes differ from the snapshot's before the restore under test."""
    eng.restore(0)
    eng.step(_odom(eng, (-0.03, 0.02, 0.3)))


def _restore_step(eng, act, active=None, odom_edit=None):
    """restore 0 -> one step; returns the inc_stats delta (incremental, full) of that step."""
    _diverge(eng)
    eng.restore(0)
    odom = _odom(eng, act)
    if odom_edit is not None:
        odom_edit(odom)
    before = eng.inc_stats()
    eng.step(odom, active)
    after = eng.inc_stats()
    return after[0] - before[0], after[1] - before[1]


JIG, GATE = (0.05, 0.0, 0.01), (2.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def inplace():
    p = Pair(LP.inplace_world(), n_roll=4)
    yield p
    p.close()


@pytest.fixture(scope="module")
def small():
    p = Pair(LP.small_world())
    yield p
    p.close()


def test_in_place_batches(inplace):
    """Panels of 68 landmarks in HBM / L2, 8 / 12 / 16 re-observed (one narrow batch, one wide batch), the ring of 48 in three batches
    (the later ones read the instance only), nf = 65: inc_post refuses with the panel in place."""
    snaps = inplace.start("jgb")
    stats = inplace.run(lambda eng: _restore_step(eng, JIG))
    assert stats[0] == stats[1] == (5, 1), stats  # (the ring of 65: a full solve)
    _assert_same(inplace, "in place", snaps)
    # ... and the steps behind it go on from the panel the update left
    inplace.run(lambda eng: eng.step(_odom(eng, (-0.05, 0.0, -0.01))))
    _assert_same(inplace, "in place, second step", snaps)


def test_in_place_first_sightings_and_refusals(inplace):
    """The gate step: (48, 4) re-observes 48 and first-sights 4 in place; the large gates and nn = 13 are refused (full solves)."""
    snaps = inplace.start("j")
    stats = inplace.run(lambda eng: _restore_step(eng, GATE))
    assert stats[0] == stats[1] == (1, 5), stats
    _assert_same(inplace, "in place, gate step", snaps)


def test_lds_staged(small):
    snaps = small.start("j")
    stats = small.run(lambda eng: _restore_step(eng, JIG))
    assert stats[0] == stats[1] == (8, 0), stats
    _assert_same(small, "lds", snaps)


def test_lds_staged_first_sightings_and_refusal(small):
    """The gate step with the panel in LDS: (8, 1) and (17, 12) first-sight their gates, nn = 13 of ring 33 is refused."""
    snaps = small.start("j")
    stats = small.run(lambda eng: _restore_step(eng, GATE))
    assert stats[0] == stats[1] == (7, 1), stats
    _assert_same(small, "lds, gate step", snaps)


def test_relinearising_step():
    pair = Pair(LP.relin_world())
    try:
        snaps = pair.start(LP.RELIN_SCRIPT[:-1])
        stats = pair.run(lambda eng: _restore_step(eng, JIG))
        assert stats[0] == stats[1] == (0, pair.world.n), stats  # every env relinearises: the full solve, panel_from_dense
        _assert_same(pair, "relinearising", snaps)
        pair.run(lambda eng: eng.step(_odom(eng, (-0.05, 0.0, -0.01))))
        _assert_same(pair, "behind the relinearising step", snaps)
    finally:
        pair.close()


@pytest.mark.parametrize("which", ["inplace", "small"])
def test_exits_without_update(which, request):
    """A rejected move and an env switched off: the step copies the panel, and the next update goes on from the copy."""
    pair = request.getfixturevalue(which)
    snaps = pair.start("jgb" if which == "inplace" else "j")
    n = pair.world.n

    def run(eng):
        active = torch.ones(n, dtype=torch.uint8, device=eng.device)
        active[1] = 0
        def edit(odom):
            odom[2, 0] = 1000.0  # outside the map: the simulator rejects the move
        return _restore_step(eng, JIG, active, edit)
    stats = pair.run(run)
    assert stats[0] == stats[1], stats
    _assert_same(pair, which + ": masked / rejected", snaps)
    stats = pair.run(lambda eng: (eng.inc_stats(), eng.step(_odom(eng, (-0.05, 0.0, -0.01))), eng.inc_stats()))
    for before, _, after in stats:
        assert after[0] - before[0] >= 2  # (the two envs the step before left alone are served from the copied panels)
    _assert_same(pair, which + ": the step behind", snaps)


@pytest.mark.parametrize("call", ["snapshot", "graph", "lookahead", "panel"])
def test_restore_then_other_call(inplace, call):
    """Entry points other than the step settle the debt first."""
    snaps = inplace.start("jgb")
    res = []
    for eng in inplace.engines:
        _diverge(eng)
        eng.restore(0)
        if call == "snapshot":
            eng.snapshot(1)
            r = [np.frombuffer(b"".join(_snapshot_bytes(eng, 1)), dtype=np.uint8)]
        elif call == "graph":
            r = [eng.graph()["x"].cpu().numpy()]
        elif call == "panel":
            r = [x for i in range(eng.n_envs) for x in eng.panel(i)]
        else:
            A = eng.cfg.max_actions
            acts = np.zeros((4, A, 3))
            acts[:, 0], acts[:, 1] = (0.05, 0.0, 0.01), (-0.05, 0.0, -0.01)
            ce = torch.tensor([0, 1, 3, 4], dtype=torch.int32, device=eng.device)
            r = [eng.lookahead(ce, torch.tensor(acts, device=eng.device), torch.tensor([2, 1, 2, 2], dtype=torch.int32, device=eng.device),
                               max_n_actions=2).cpu().numpy()]
        eng.step(_odom(eng, JIG))
        res.append(r)
    for x, y in zip(*res):
        assert x.tobytes() == y.tobytes(), call
    _assert_same(inplace, "restore, %s, step" % call, snaps)


def test_stacked_and_repeated_restores(inplace):
    snaps = inplace.start("jgb")

    def run(eng):
        _diverge(eng)
        eng.restore(0)
        eng.restore(0)
        eng.step(_odom(eng, JIG))
        eng.snapshot(1)
        eng.step(_odom(eng, (-0.05, 0.0, -0.01)))
        eng.restore(1)  # (another slot than the one the first debt named)
        eng.step(_odom(eng, (0.02, 0.01, 0.0)))
        eng.restore(0)
        eng.step(_odom(eng, JIG))
        eng.step(_odom(eng, (-0.05, 0.0, -0.01)))
    inplace.run(run)
    _assert_same(inplace, "stacked restores", snaps)


@pytest.mark.parametrize("which", ["inplace", "small"])
def test_stage_kernels(which, request):
    """timing_enable(2): the three stage kernels know one panel base; they copy the body first."""
    pair = request.getfixturevalue(which)
    snaps = pair.start("jgb" if which == "inplace" else "j")

    def run(eng):
        eng.timing_enable(2)
        try:
            return _restore_step(eng, JIG)
        finally:
            eng.timing_enable(False)
            eng.timing_read()
    stats = pair.run(run)
    assert stats[0] == stats[1], stats
    _assert_same(pair, which + ": stage kernels", snaps)
    fused = pair.run(lambda eng: (_restore_step(eng, JIG), _state(eng))[1])
    staged = pair.run(lambda eng: (run(eng), _state(eng))[1])
    for x, y in zip(fused[1], staged[1]):
        assert x.tobytes() == y.tobytes(), which + ": staged against fused"


def test_pose_chain_kernels():
    """Beyond 53 poses: the fused step around the pose-chain solver (streamed and two-walk updates) copies the body first."""
    pair = Pair(LP.chain_world())
    try:
        snaps = pair.start(LP.CHAIN_SCRIPT)
        stats = pair.run(lambda eng: _restore_step(eng, JIG))
        assert stats[0] == stats[1] and stats[0][0] + stats[0][1] == pair.world.n, stats
        _assert_same(pair, "pose chain", snaps)
    finally:
        pair.close()
