"""GPU tests of the compact restore (csrc/k_misc.hip: k_restore_compact, a lazy drlgx_restore by one workgroup per environment): an
engine created with DRLGX_RESTORE_COMPACT=1 and one created with =0 (the generic copy kernel) are driven through the same calls on
the cases of tests/restore_compact_cases.py and must agree BIT FOR BIT - counts, estimates, information blocks, covariance traces,
factor lists, ground truth, the virtual map, the covariance panel (header and live extent), utility, metrics and status - right
behind the restore (the getters settle what it owes) and behind the steps that follow it; the snapshot stays byte for byte what it was."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lazy_panel_cases as LP  # noqa: E402
import restore_compact_cases as RC  # noqa: E402

SWITCHES = ("DRLGX_RESTORE_COMPACT", "DRLGX_RESTORE_EAGER", "DRLGX_INCREMENTAL")
JIG, BACK = (0.05, 0.0, 0.01), (-0.05, 0.0, -0.01)


def _engine(case, compact, eager=False, incremental=True, n_roll=0):
    from drl_graph_exploration_amd.engine import Engine
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ["DRLGX_RESTORE_COMPACT"] = "1" if compact else "0"
        if eager:
            os.environ["DRLGX_RESTORE_EAGER"] = "1"
        if not incremental:
            os.environ["DRLGX_INCREMENTAL"] = "0"
        eng = Engine(case.engine_config(max_snapshots=2), case.world.n, n_roll)  # (the switches are read once, when the engine is created)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    eng.set_fixed_landmarks(case.world.fixed)
    return eng


def _odom(eng, act):
    return torch.tensor(np.array([act] * eng.n_envs, dtype=np.float64), device=eng.device)


def _instance(eng, i):
    c = eng.counts(i)
    out = [np.array([c[k] for k in sorted(c)])]
    out += list(eng.poses(i)) + list(eng.landmarks(i)) + list(eng.cov_traces(i)) + list(eng.factors(i)) + list(eng.ground_truth(i))
    out += [np.asarray(v) for v in eng.virtual_map(i)]
    meta, body = eng.panel(i)
    out.append(meta)
    if body is not None:
        out.append(body)
    return out


def _state(eng):
    out = [np.array([eng.status()]), eng.utility().cpu().numpy(), eng.metrics().cpu().numpy()]
    for i in range(eng.n_envs):
        out += _instance(eng, i)
    return out


def _snapshot_bytes(eng, slot):
    return [x.tobytes() for e in range(eng.n_envs) for x in _instance(eng, eng.snapshot_instance(slot, e))]


class Pair(object):
    """The compact and the generic engine of one case (or any two engines that must agree)."""

    def __init__(self, case, n_roll=0, incremental=True, engines=None):
        self.case = case
        self.engines = engines or (_engine(case, True, incremental=incremental, n_roll=n_roll), _engine(case, False, incremental=incremental, n_roll=n_roll))

    def close(self):
        for eng in self.engines:
            eng.close()

    def run(self, fn):
        return [fn(eng) for eng in self.engines]

    def start(self, slot=0, before_snapshot=None):
        """Both engines: reset, the case's script under its activity masks, snapshot `slot`.  Returns the snapshot's bytes (per engine)."""
        case, n = self.case, self.case.world.n
        for eng in self.engines:
            eng.reset(np.arange(n), np.arange(n), starts=case.world.starts)
            for s, a in enumerate(LP.actions(case.script, n)):
                eng.step(torch.tensor(a, device=eng.device), torch.tensor(case.active(s), device=eng.device))
            if before_snapshot is not None:
                before_snapshot(eng)
            eng.snapshot(slot)
        return [_snapshot_bytes(eng, slot) for eng in self.engines]

    def same(self, what, snaps=None, slot=0, status=0):
        a, b = self.run(_state)
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: item %d differs" % (what, k)
        if status is not None:
            assert int(a[0][0]) == status, what
        if snaps is not None:  # the snapshot is read-only
            for eng, before in zip(self.engines, snaps):
                assert _snapshot_bytes(eng, slot) == before, what + ": the snapshot changed"


def _diverge(eng, slot=0):
    """One other step away from the snapshot: what the restore under test leaves behind cannot pass unnoticed."""
    eng.restore(slot)
    eng.step(_odom(eng, (-0.03, 0.02, 0.3)))


def _restore_checks(pair, snaps, what, slot=0, status=0):
    """Right behind the restore (the getters settle its debt), behind the step that follows a restore, and one step further."""
    pair.run(lambda eng: (_diverge(eng, slot), eng.restore(slot)))
    pair.same(what + ": restored", snaps, slot, status)
    for eng, before in zip(pair.engines, snaps):  # ... and the envs ARE the snapshot
        assert [x.tobytes() for e in range(eng.n_envs) for x in _instance(eng, e)] == before, what
    pair.run(lambda eng: (_diverge(eng, slot), eng.restore(slot), eng.step(_odom(eng, JIG))))
    pair.same(what + ": restore, step", snaps, slot, status)
    pair.run(lambda eng: eng.step(_odom(eng, BACK)))
    pair.same(what + ": restore, two steps", snaps, slot, status)


def _table_items(eng, inst):
    """(16-byte items, words) the restore of instance `inst` moves, from the engine's own table and the instance's counts."""
    info, rows = eng.restore_table()
    c = eng.counts(inst)
    meta = eng.panel(inst)[0]
    table = [(int(r[0]), int(r[1]), int(r[2])) for r in rows]
    assert all(int(r[3]) == 0 for r in rows)  # (no sub-slice entries among what a lazy restore copies)
    return RC.instance_items(table, (c["poses"], c["landmarks"], c["factors"]), int(meta[1]) if meta[0] == 1 else 0), info


def _counts(eng):
    return [tuple(eng.counts(i)[k] for k in ("poses", "landmarks", "factors")) for i in range(eng.n_envs)]


@pytest.fixture(scope="module")
def mixed():
    p = Pair(RC.mixed_case(), n_roll=4)
    yield p
    p.close()


def test_table_and_switches(mixed):
    """The engines' own words: which kernel a restore launches, and that the table is the field list the CPU tests restate."""
    case = mixed.case
    (info1, rows1), (info0, rows0) = mixed.run(lambda eng: eng.restore_table())
    assert info1["in_use"] and not info0["in_use"]
    assert rows1.tobytes() == rows0.tobytes() and info1["entries"] == len(rows1) <= 32
    want = sorted((stride, unit, ub) for _, stride, unit, ub in RC.rows(case.caps(), case.world.num_landmarks))
    assert sorted((int(r[0]), int(r[1]), int(r[2])) for r in rows1) == want
    kinds = [int(r[0]) % 16 == 0 for r in rows1]
    assert kinds == [True] * info1["entries_16"] + [False] * (info1["entries"] - info1["entries_16"])
    assert info1["items_per_trip"] == 512 * 4


def test_empty_and_odd_instances(mixed):
    """One engine, four counts: a just-reset env without a landmark, L = M = 1, and L = 3 / 5 with odd M (4-byte entries off the 16-byte grid)."""
    snaps = mixed.start()
    assert mixed.run(_counts) == [RC.MIXED_COUNTS] * 2
    _restore_checks(mixed, snaps, "mixed")


def test_slot_1_and_repeated_restores(mixed):
    snaps1 = mixed.start(slot=1)

    def run(eng):
        eng.step(_odom(eng, JIG))
        eng.snapshot(0)  # slot 0: one step further than slot 1
        _diverge(eng, 1)
        eng.restore(0)
        eng.restore(1)  # restore, restore again - another slot than the first debt named -, step
        eng.step(_odom(eng, JIG))
    mixed.run(run)
    mixed.same("restore 0, restore 1, step", snaps1, slot=1)
    _restore_checks(mixed, snaps1, "slot 1", slot=1)


@pytest.mark.parametrize("call", ["lookahead", "cov_array", "snapshot"])
def test_restore_then_other_call(mixed, call):
    """Entry points other than the step settle what the compact restore owes, as they do behind the generic one."""
    snaps = mixed.start()
    res = []
    for eng in mixed.engines:
        _diverge(eng)
        eng.restore(0)
        if call == "snapshot":
            eng.snapshot(1)
            r = [np.frombuffer(b"".join(_snapshot_bytes(eng, 1)), dtype=np.uint8)]
        elif call == "cov_array":
            r = [t.cpu().numpy() for t in eng.cov_array()]
        else:
            acts = np.zeros((3, eng.cfg.max_actions, 3))
            acts[:, 0], acts[:, 1] = JIG, BACK
            ce = torch.tensor([0, 2, 3], dtype=torch.int32, device=eng.device)
            r = [eng.lookahead(ce, torch.tensor(acts, device=eng.device), torch.tensor([2, 1, 2], dtype=torch.int32, device=eng.device),
                               max_n_actions=2).cpu().numpy()]
        eng.step(_odom(eng, JIG))
        res.append(r)
    for x, y in zip(*res):
        assert x.tobytes() == y.tobytes(), call
    mixed.same("restore, %s, step" % call, snaps)


def test_subset_reset_between_snapshot_and_restore(mixed):
    """The reset draws other ground-truth landmarks: the restore brings the snapshot's back (the class-2 entry)."""
    snaps = mixed.start()
    world = mixed.case.world

    def run(eng):
        _diverge(eng)
        eng.set_fixed_landmarks(world.fixed + 0.125)
        eng.reset(np.array([1, 3]), np.array([7, 9]), starts=world.starts[[1, 3]])
        # (the getter reads the landmarks of the instance's parent - for a snapshot instance the live env: compare with the lists)
        assert np.array_equal(eng.ground_truth(3)[1], world.fixed + 0.125) and not np.array_equal(world.fixed + 0.125, world.fixed)
        eng.set_fixed_landmarks(world.fixed)
        eng.restore(0)
        eng.step(_odom(eng, JIG))
        for e in range(eng.n_envs):
            assert eng.ground_truth(e)[1].tobytes() == np.ascontiguousarray(world.fixed, dtype=np.float64).tobytes()
    mixed.run(run)
    mixed.same("subset reset, restore, step", snaps)


def test_invalid_panel_at_snapshot_time(mixed):
    """Env 1 is reset by stages right before the snapshot (no solve: its panel's header says invalid); envs 2 / 3 hold valid panels."""
    def staged(eng):
        on = torch.tensor(np.array([0, 1, 0, 0], dtype=np.uint8), device=eng.device)
        eng.stage_reset([1], [5], mixed.case.world.starts[[1]])
        k, br, c = eng.stage_measure(on)
        eng.stage_add_measurements(k, br, c, on)
    snaps = mixed.start(before_snapshot=staged)
    for eng in mixed.engines:
        valid = [int(eng.panel(eng.snapshot_instance(0, e))[0][0]) for e in range(eng.n_envs)]
        assert valid[1] == 0 and valid[2] == valid[3] == 1, valid
    _restore_checks(mixed, snaps, "invalid panel", status=None)


def test_engine_without_panels():
    pair = Pair(RC.mixed_case(), incremental=False)
    try:
        assert all(eng.inc_stats() == (-1, -1) for eng in pair.engines)
        (info, rows), _ = pair.run(lambda eng: eng.restore_table())
        assert info["in_use"] and not any(int(r[1]) == 4 for r in rows)  # (no pose marginals of a panel in the table)
        snaps = pair.start()
        _restore_checks(pair, snaps, "no panels")
    finally:
        pair.close()


def test_eager_flag_keeps_the_generic_kernel():
    """DRLGX_RESTORE_EAGER=1: the full copy, by the generic kernel whatever DRLGX_RESTORE_COMPACT says - and the same belief."""
    case = RC.mixed_case()
    pair = Pair(case, engines=(_engine(case, True, eager=True), _engine(case, False)))
    try:
        assert not pair.engines[0].restore_table()[0]["in_use"]
        snaps = pair.start()
        _restore_checks(pair, snaps, "eager")
    finally:
        pair.close()


def test_at_capacity():
    """P == max_poses, L == max_landmarks, M == max_factors: live == stride, the rounded-up byte counts are cut back to the slice."""
    pair = Pair(RC.capacity_case())
    try:
        snaps = pair.start()
        assert pair.run(_counts) == [RC.CAPACITY_COUNTS] * 2
        # (no further pose fits, so a step cannot move the envs away from the snapshot: another episode does)
        n, world = pair.case.world.n, pair.case.world

        def other_episode(eng):
            eng.reset(np.arange(n), 100 + np.arange(n), starts=world.starts)
            eng.step(_odom(eng, JIG))
        pair.run(lambda eng: (other_episode(eng), eng.restore(0)))
        pair.same("capacity: restored", snaps)
        for eng, before in zip(pair.engines, snaps):
            assert [x.tobytes() for e in range(eng.n_envs) for x in _instance(eng, e)] == before
        # ... and the step behind the restore reports the capacity status, the same in both engines
        pair.run(lambda eng: (other_episode(eng), eng.restore(0), eng.step(_odom(eng, JIG))))
        pair.same("capacity: restore, step", snaps, status=None)
        assert all(eng.status() != 0 for eng in pair.engines)
    finally:
        pair.close()


def test_loop_wrap():
    """The ring of 33 after 55 steps: 3 143 16-byte items and 4 085 words - more than one trip of the loop (512 threads x 4 and x 2) -
    beside an instance of 4 poses that fills less than half of one."""
    pair = Pair(RC.wrap_case())
    try:
        snaps = pair.start()
        assert pair.run(_counts) == [RC.WRAP_COUNTS] * 2
        eng = pair.engines[0]
        (q, w), info = _table_items(eng, eng.snapshot_instance(0, 2))
        assert (q, w) == (3143, 4085) and q > info["items_per_trip"] and w > info["items_per_trip"] // 2
        (q0, w0), _ = _table_items(eng, eng.snapshot_instance(0, 0))
        assert q0 < info["items_per_trip"] // 2 and w0 < info["items_per_trip"] // 4
        _restore_checks(pair, snaps, "wrap")
    finally:
        pair.close()
