"""CPU tests of what tests/test_gpu_restore_compact.py takes for granted: that the open-loop scripts of tests/restore_compact_cases.py
give the counts its cases are named for (the CPU oracle), that those counts sit on the edges claimed (empty slices, 4-byte entries that
end off a 16-byte boundary, live == stride, more items than one trip of the kernel's loop), and that the library's live-byte formula
(drlgx_debug_field_live_bytes: what every copy kernel and the host use) is the generic copy kernel's arithmetic as restated there."""
import pytest

import lazy_panel_cases as LP
import restore_compact_cases as RC

CASES = {"mixed": (RC.mixed_case, RC.MIXED_COUNTS), "wrap": (RC.wrap_case, RC.WRAP_COUNTS), "capacity": (RC.capacity_case, RC.CAPACITY_COUNTS)}
# one trip of the 512-thread kernel: 4 loads of 16 bytes and 2 of a word in flight per thread (k_misc.hip); the 256- and 1024-thread
# variants move 1 024 / 4 096 and 512 / 2 048
TRIP_16, TRIP_WORDS = 512 * 4, 512 * 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_scripts_give_the_counts(name):
    case, want = CASES[name][0](), CASES[name][1]
    sims = case.world.make_sims()
    for s, acts in enumerate(LP.actions(case.script, case.world.n)):
        on = case.active(s)
        for e, sim in enumerate(sims):
            if on[e]:
                sim.simulate(tuple(acts[e]))
    got = [(len(sim.poses()[0]), len(sim.landmarks()[0]), len(sim.factors()[0])) for sim in sims]
    assert got == want


def _lib():
    from drl_graph_exploration_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(CASES))
def test_live_bytes_are_the_generic_formula(name):
    case, counts = CASES[name][0](), CASES[name][1]
    L = _lib()
    for c in counts + [(0, 0, 0), (-1, -3, -2)]:
        for panel_poses in (0, c[0]):
            for n, stride, unit, unit_bytes in RC.rows(case.caps(), case.world.num_landmarks):
                k = RC.count_of(unit, c, panel_poses)
                want = RC.live_bytes(stride, unit, unit_bytes, k)
                assert L.drlgx_debug_field_live_bytes(stride, unit, unit_bytes, 0, k) == want, (name, n, c)
                assert want <= stride and (want % 16 == 0 or want == stride)
    # a sub-slice entry (pad) stands for its own bytes, whatever the counts
    assert L.drlgx_debug_field_live_bytes(4800, 0, 0, 1600, 7) == 1600


def test_mixed_case_edges():
    case = RC.mixed_case()
    rows = {n: (stride, unit, ub) for n, stride, unit, ub in RC.rows(case.caps(), case.world.num_landmarks)}
    # the instance that was just reset: every per-landmark / per-factor entry is empty
    for n, (stride, unit, ub) in rows.items():
        if unit in (2, 3):
            assert RC.live_bytes(stride, unit, ub, RC.count_of(unit, RC.MIXED_COUNTS[0], 1)) == 0, n
    # the 4-byte entries of envs 2 and 3 end off a 16-byte boundary: the copy rounds up
    for c in RC.MIXED_COUNTS[2:]:
        assert c[1] in (3, 5) and c[2] % 2 == 1
        for n in ("lm_key", "meas_pose", "meas_lm"):
            stride, unit, ub = rows[n]
            k = RC.count_of(unit, c, c[0])
            assert (k * 4) % 16 != 0 and RC.live_bytes(stride, unit, ub, k) == (k * 4 + 15) // 16 * 16
    # both item kinds occur among the entries with live bytes
    assert rows["lm_key"][0] % 16 != 0 and rows["meas_pose"][0] % 16 == 0


def test_capacity_case_is_at_capacity():
    case = RC.capacity_case()
    caps = case.caps()
    assert RC.CAPACITY_COUNTS[0] == (caps["max_poses"], caps["max_landmarks"], caps["max_factors"])
    for n, stride, unit, ub in RC.rows(caps, case.world.num_landmarks):
        if unit:  # live == stride: the clamp (77 keys x 4 bytes = 308, rounded up to 320, are cut back to the slice)
            assert RC.live_bytes(stride, unit, ub, RC.count_of(unit, RC.CAPACITY_COUNTS[0], 8)) == stride, n
    assert (77 * 4 + 15) // 16 * 16 > 77 * 4


def test_wrap_case_wraps_the_loop():
    case = RC.wrap_case()
    table = [(stride, unit, ub) for _, stride, unit, ub in RC.rows(case.caps(), case.world.num_landmarks)]
    q, w = RC.instance_items(table, RC.WRAP_COUNTS[2], RC.WRAP_COUNTS[2][0])
    assert (q, w) == (3143, 4085)  # 16-byte items and words of the ring of 33 (2 x 1 848 of the words are its factor lists)
    assert q > TRIP_16 and w > TRIP_WORDS
    q0, w0 = RC.instance_items(table, RC.WRAP_COUNTS[0], RC.WRAP_COUNTS[0][0])
    assert q0 < TRIP_16 // 2 and w0 < TRIP_WORDS // 2  # the short instance: less than half a trip of either kind
