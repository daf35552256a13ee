"""CPU tests of what tests/test_gpu_lazy_panel.py takes for granted: that the worlds of tests/lazy_panel_cases.py put their panels on
the forms of the incremental update they are named for (step_cases.inc_form, the restatement of inc_plan's arithmetic that
tests/test_step_cpu.py checks), and that their open-loop scripts give the counts the forms are computed from (the CPU oracle)."""
import numpy as np
import pytest

import lazy_panel_cases as LP
import step_cases as S

WORLDS = {"inplace": LP.inplace_world, "small": LP.small_world}


def test_forms_table():
    for (wname, ring, P), want in LP.FORMS.items():
        world = WORLDS[wname]()
        e = [r[0] for r in world.rings].index(ring)
        gate_seen = wname == "inplace" and P == 5
        assert LP.form(world, e, P, ring, gate_seen) == want, (wname, ring, P)


def test_inplace_panels_never_fit_the_lds():
    world = LP.inplace_world()
    for e, (size, gate) in enumerate(world.rings):
        for P in range(2, world.caps["max_poses"] + 1):
            if size + gate >= 52:
                assert LP.form(world, e, P, size, True).startswith("two-walk"), (size, P)


@pytest.mark.parametrize("wname,script", [("inplace", LP.INPLACE_SCRIPT), ("small", "jg")])
def test_open_loop_scripts_give_the_counts(wname, script):
    """Landmarks in range, factors appended and first sightings of every step, against step_cases' closed-loop expectation."""
    world = WORLDS[wname]()
    sims = world.make_sims()
    want = world.expected_counts(script)
    for s, acts in enumerate(LP.actions(script, world.n)):
        for e, sim in enumerate(sims):
            L0, M0 = len(sim.landmarks()[0]), len(sim.factors()[0])
            sim.simulate(tuple(acts[e]))
            nf, nn = len(sim.factors()[0]) - M0, len(sim.landmarks()[0]) - L0
            assert (nf, nf - nn, nn) == want[s + 1][e][1:], (wname, s, world.rings[e])


def test_relin_world_relinearises_at_its_last_step():
    world = LP.relin_world()
    sims = world.make_sims()
    acts = LP.actions(LP.RELIN_SCRIPT, world.n)
    for a in acts[:-1]:
        for e, sim in enumerate(sims):
            sim.simulate(tuple(a[e]))
    assert all(S.relinearises(sim)[0] for sim in sims)
