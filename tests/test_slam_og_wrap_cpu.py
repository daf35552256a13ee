"""What tests/test_gpu_slam_og_wrap.py requires of the cases of tests/slam_og_wrap_cases.py, checked on the CPU with the
restatement tests/slam_og_ref.py alone.  No GPU.  These are conditions: they keep the GPU test from passing for the wrong reason.

  * the corridor has P + L = 280 > 256 owners, L = 270 > 256 slots, P = max_poses; every case predicts the number of measurements
    of its table; the cap cases exactly 256; the overflows more; the masked overflow no more;
  * for every case with a predicted measurement, the restatement's information form and its covariance-form downdate agree to
    1e-3 of the tolerance the GPU test gives a block (rtol 1e-6 / atol 1e-10): the kernel keeps the other 99.9 %;
  * a wrong or missing update would show: every slot >= 246 of `corridor_end` (the second-trip owners of the ordered prior) and
    every slot of the cap cases lies more than 100 tolerances off the prior; dropping the mask of `corridor_core9` moves a block by
    more than 100 tolerances;
  * no predicted pair sits within 1e-6 of a gate (fm2_cases.predicted_pairs, as tests/test_fm2_cpu.py requires of its own).

Measured here, information form against downdate as a share of the block tolerance: fresh_K8 9.7e-7, walked_K8 6.0e-7,
ring65_K2 9.0e-7, ring17_K1 8.9e-8, corridor_end 1.3e-6, corridor_core9 3.5e-6, corridor_back 3.5e-5.
"""
import numpy as np
import pytest

import fm2_cases as F
import slam_og_ref as R
import slam_og_wrap_cases as W

_ALL = [(w, c) for w in sorted(W.CASES) for c in sorted(W.CASES[w])]
_SEEN = [(w, c) for w, c in _ALL if W.CASES[w][c][3] > 0]
SECOND_TRIP_SLOT = 256 - F.CORRIDOR_CAPS["max_poses"]   # owner o = P + slot: slots >= 246 are a thread's second owner


@pytest.fixture(scope="module")
def worlds():
    return {name: W.world(name) for name in W.CASES}


@pytest.fixture(scope="module")
def blocks(worlds):
    """(information form, downdate, prior) landmark blocks of a case, computed once."""
    made = {}

    def get(wname, case):
        if (wname, case) not in made:
            e, plan, core, _ = W.CASES[wname][case]
            sim = worlds[wname].sims[e]
            made[wname, case] = (R.landmark_blocks(sim, plan, core)[0], R.landmark_blocks_downdate(sim, plan, core),
                                 R.prior_landmark_blocks(sim))
        return made[wname, case]
    return get


def _tolerances(got, want):
    """|got - want| in units of the GPU test's tolerance of that element, per slot (the largest of its block)."""
    return (np.abs(got - want) / (W.LM_RTOL * np.abs(want) + W.LM_ATOL)).reshape(len(want), -1).max(axis=1)


def test_the_corridor_wraps_every_loop(worlds):
    sim = worlds["corridor"].sims[0]
    P, L = sim.num_poses(), sim.num_landmarks()
    assert (P, L) == (10, 270) and P == F.CORRIDOR_CAPS["max_poses"]
    assert P + L == 280 > 256 and L > 256 and L > 4 * 64
    assert SECOND_TRIP_SLOT == 246 and L - SECOND_TRIP_SLOT == 24
    assert [s.num_landmarks() for s in worlds["rings"].sims] == F.RING_SIZES
    rows, cols = sim.vm_shape()
    assert rows * cols == 1600 and worlds["rings"].sims[0].vm_shape() == (rows, cols)


def test_counts(worlds):
    for wname, case in _ALL:
        e, plan, core, nm = W.CASES[wname][case]
        assert W.predicted(worlds[wname].sims[e], plan, core) == nm <= W.MAX_MEAS, case
        assert len(plan) <= worlds[wname].caps["max_actions"]
    for name in W.AT_THE_CAP:
        assert W.CASES["rings"][name][3] == 256 == W.MAX_MEAS
    want = {"corridor_K0": 0, "corridor_end": 172, "corridor_back": 228, "corridor_core9": 130, "corridor_blind": 0, "fresh_K8": 256,
            "walked_K8": 256, "walked_K1": 32, "ring65_K2": 130, "ring33_K1": 33, "ring16_K1": 16, "ring17_K1": 17, "fresh_K0": 0,
            "walked_K0": 0}
    assert {c: W.CASES[w][c][3] for w, c in _ALL} == want
    assert len(W.CASES["corridor"]["corridor_blind"][1]) == 1 and len(W.CORE9_PLAN) == 9 == F.CORRIDOR_CAPS["max_actions"]
    for wname, (e, plan, core) in W.OVERFLOWS.items():
        assert W.predicted(worlds[wname].sims[e], plan, core) > W.MAX_MEAS, wname
    e, plan, core, nm = W.MASKED_OVERFLOW
    assert plan == W.OVERFLOWS["corridor"][1] and core == [1, 0, 1, 0]
    assert 0 < W.predicted(worlds["corridor"].sims[e], plan, core) == nm <= W.MAX_MEAS
    # the masked plan's measurements reach the slots behind the compaction's first pass of 256
    seen = [p[1] for p in F.predicted_pairs(worlds["corridor"].sims[0], W.CORE9_PLAN)[0] if p[4] and W.CORE9_MASK[p[0]]]
    assert len(seen) == 130 and max(seen) >= 256


def test_no_new_plan_sits_on_a_gate(worlds):
    """The corridor's named plans and both overflows are tests/test_fm2_cpu.py's; the masked and the blind plan are new here.  (The
    margin is taken over every pose of the plan, masked out or not.)"""
    sim = worlds["corridor"].sims[0]
    for name, plan in (("corridor_core9", W.CORE9_PLAN), ("corridor_blind", [W.BLIND]), ("masked overflow", W.MASKED_OVERFLOW[1])):
        margin = F.predicted_pairs(sim, plan)[1]
        print("%s: smallest gate margin %.3e" % (name, margin))
        assert margin > 1e-6, "%s sits on a knife edge (%.3e): choose another plan" % (name, margin)


@pytest.mark.parametrize("wname,case", _SEEN, ids=[c for _, c in _SEEN])
def test_two_routes_agree_and_the_update_shows(blocks, wname, case):
    info, down, prior = blocks(wname, case)
    gap = _tolerances(down, info).max()
    moved = _tolerances(prior, info)
    line = "%s: nm %d  information form against downdate %.2e of the block tolerance; off the prior: every slot >= %.2e tolerances" % (
        case, W.CASES[wname][case][3], gap, moved.min())
    if len(moved) > SECOND_TRIP_SLOT:
        line += ", slots >= %d >= %.2e" % (SECOND_TRIP_SLOT, moved[SECOND_TRIP_SLOT:].min())
    print(line)
    assert gap <= 1e-3, case
    assert moved.max() >= 100.0, case
    if case in W.AT_THE_CAP:
        assert moved.min() >= 100.0, case
    if case == "corridor_end":
        assert len(moved[SECOND_TRIP_SLOT:]) == 24 and moved[SECOND_TRIP_SLOT:].min() >= 100.0


def test_the_mask_of_core9_is_not_inert(worlds, blocks):
    e, plan, core, nm = W.CASES["corridor"]["corridor_core9"]
    sim = worlds["corridor"].sims[e]
    bare, n_meas = R.landmark_blocks(sim, plan, None)
    assert sum(n_meas) > W.MAX_MEAS > nm                       # (the restatement has no cap)
    assert _tolerances(bare, blocks("corridor", "corridor_core9")[0]).max() >= 100.0


def test_a_blind_plan_keeps_the_prior(worlds):
    """`corridor_blind` and `corridor_K0`: no measurement, so the restatement's blocks are the prior's (another matrix is inverted:
    not the same bits) and w1 * slam_uncertainty = alpha."""
    for case in ("corridor_blind", "corridor_K0"):
        ref = W.reference(worlds["corridor"], case)
        prior = R.prior_landmark_blocks(worlds["corridor"].sims[0])
        assert ref["nm"] == 0
        assert _tolerances(ref["lm_cov"], prior).max() <= 1e-3, case
        assert ref["w1"] * ref["slam_uncertainty"] == pytest.approx(W.ALPHA, rel=1e-9), case
