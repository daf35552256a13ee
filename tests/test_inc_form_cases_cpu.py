"""CPU checks, with the oracle alone, that the worlds of tests/inc_form_cases.py are what they claim - before
tests/test_gpu_inc_forms.py relies on them on the device.  For every case, at the check step and at the EXTRA steps behind it:

  D1  the counts: poses after the step, L0 landmarks in the panel before it, n_re re-observed landmarks, no first sighting (<= INEW =
      12 would do), at most INF = 64 new factors, no landmark twice;
  D2  no relinearisation is due at that step (step_cases.relinearises);
  D3  over the whole script no true or measured range / bearing lies within 1e-6 of a sensor limit (range, bearing gate = field of view);
  D4  step_cases.inc_form - the restated plan arithmetic, at the pose bound of the launch the GPU test will make - puts the case in
      its cell.

Measured here (printed with -s): smallest margin 0.24 (m or rad); the six walks take 0.1 .. 5 s (chain270b: 230 landmarks, 56 poses).
"""
import pytest

import inc_form_cases as F
import step_cases as S

WORLDS = {w.name: w for w in F.worlds()}


def calls_before(world, s, e):
    """drlgx_step calls the GPU test has made before it steps environment e at step s >= check_step: every environment together up to
    the check step, one at a time from there."""
    return world.check_step + (s - world.check_step) * world.n + e


@pytest.mark.parametrize("name,wname,e,cell", F.CASES, ids=[c[0] for c in F.CASES])
def test_case_is_in_its_cell(name, wname, e, cell):
    world = WORLDS[wname]
    run = F.walk(world)
    print("\n%s: world %s (%d listed landmarks, capacities %s), environment %d, smallest margin %.3e" % (
        name, wname, world.num_landmarks, world.caps, e, run["margin"]))
    assert run["margin"] >= 1e-6                                                                    # D3
    for s in range(world.check_step, world.check_step + 1 + F.EXTRA):
        P, L0, nf, n_re, nn, relin, distinct = run["rows"][s][e]
        assert (P, L0, n_re, nn) == world.expected(e, s), (s, run["rows"][s][e])                    # D1
        assert nn <= S.INEW and nf <= S.INF and distinct
        assert not relin                                                                            # D2
        assert S.expected_path((nf, nf, n_re, nn), s + 2, relin) == "inc"
        pc = F.pose_bound(world, calls_before(world, s, e))
        form = F.restated_form(world, P, L0, n_re, pc)
        print("  step %d: %d poses, L0 %d, n_re %d, pose bound %d: %s" % (s, P, L0, n_re, pc, form))
        assert form == cell, (s, form)                                                              # D4
    if name in F.BATCHES:
        assert (run["rows"][world.check_step][e][3] + 7) // 8 == F.BATCHES[name]


def test_the_cases_cover_the_cells():
    cells = {(c[3], c[1].startswith("chain")) for c in F.CASES}
    assert cells >= {("lds narrow", False), ("lds narrow", True), ("two-walk narrow", False), ("two-walk narrow", True),
                     ("streamed 1", True), ("streamed 2", True), ("streamed 2+1", True), ("streamed 1+1", True),
                     ("streamed 1+1+1", True), ("none", False)}
    assert sorted(F.BATCHES.values()) == [1, 2, 3]
    # the gate step that takes the field in is a full solve: more than INF factors or more than INEW first sightings
    for w in F.worlds():
        for size, gate in w.rings:
            assert gate == 0 or gate > S.INEW
        assert (w.check_step + 2 > S.DENSE_MAX_POSES) == w.name.startswith("chain")
