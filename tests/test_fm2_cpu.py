"""What tests/test_gpu_fm2.py requires of the cases of tests/fm2_cases.py, checked on the CPU with the restatement alone, before
any of them is run on the device.  No GPU.

  C1  every case predicts exactly the number of measurements it is named for; the corridor holds more than 256 landmarks and a
      predicted measurement to a slot >= 256;
  C2  no predicted (pose, landmark) pair lies within 1e-6 of a range or bearing gate (nothing is skipped or masked);
  C3  the restatement with its update term dropped (Sigma' = base) lies more than 100 x the GPU test's tolerance away from the
      restatement, for every parity case, and a parity case exists in every band of nm and in the corridor;
  C4  the restatement's own spread: against the same update evaluated in information form on a prior assembled from the factor
      lists, with Cholesky solves and no inverse (fm2_cases.reference_information_form).

Measured here (C3 in units of the GPU tolerance rtol 1e-6 / atol 1e-10, over all compared blocks | over the old poses' blocks;
C4 as max |Sigma'_1 - Sigma'_2| and max |Delta_1 - Delta_2|, absolute, and the latter relative to max |Delta_1|):

    case            nm   C3 all    C3 old     C4 Sigma'   C4 Delta    relative
    em_plan0        13   5.9e+06   4.4e+04    8.7e-16     8.1e-16     2.0e-14
    em_plan1         7   3.1e+06   2.4e+04    3.2e-16     2.7e-16     1.3e-14
    em_plan2        15   8.3e+06   2.9e+04    1.5e-15     1.2e-15     2.0e-14
    ring16_K1       16   1.2e+07   1.4e+06    1.1e-15     1.1e-15     3.2e-14
    ring17_K1       17   1.2e+07   1.4e+06    6.8e-16     5.4e-16     1.6e-14
    fresh_K1        32   3.8e+06   5.7e-08    2.9e-16     2.6e-16     2.6e-14
    walked_K1       32   1.3e+07   1.4e+06    1.9e-15     1.8e-15     5.6e-14
    ring33_K1       33   1.3e+07   1.4e+06    9.9e-16     7.4e-16     2.3e-14
    fresh_K2        64   7.6e+06   3.3e-08    5.2e-16     6.0e-16     3.0e-14
    walked_K2       64   1.6e+07   1.4e+06    5.5e-15     5.6e-15     1.3e-13
    ring65_K1       65   1.3e+07   1.4e+06    5.8e-15     4.2e-15     1.3e-13
    ring33_K2       66   1.6e+07   1.4e+06    4.0e-15     4.0e-15     9.3e-14
    fresh_K3        96   1.1e+07   1.1e-07    2.8e-15     2.9e-15     9.8e-14
    walked_K3       96   2.0e+07   1.4e+06    6.4e-15     6.8e-15     1.3e-13
    fresh_K4       128   1.5e+07   7.5e-08    1.5e-15     1.6e-15     4.0e-14
    walked_K4      128   2.4e+07   1.4e+06    2.2e-14     2.2e-14     3.5e-13
    ring65_K2      130   1.6e+07   1.4e+06    1.6e-14     1.4e-14     3.4e-13
    fresh_K5       160   1.9e+07   5.5e-08    5.7e-15     5.7e-15     1.1e-13
    walked_K5      160   2.8e+07   1.4e+06    1.9e-14     1.9e-14     2.6e-13
    corridor_end   172   7.6e+06   4.4e+03    3.7e-15     4.1e-15     2.1e-13
    corridor_back  228   8.9e+06   6.4e+04    7.2e-15     7.4e-15     3.2e-13
    fresh_K8       256   3.0e+07   1.9e-07    2.0e-14     2.0e-14     2.5e-13
    walked_K8      256   3.9e+07   1.4e+06    5.7e-14     5.7e-14     5.5e-13

Every case with a predicted measurement is a parity case under C3: a new pose's covariance is the odometry chain's before the
update and a landmark fix after it.  The old poses' blocks alone would not carry the `fresh` cases (the belief straight after the
reset: their update term is 1e-7 of the tolerance); they do carry the walked rings, the corridor and the em_cases belief, where
the plan closes a loop - that is required below as well, so that an update term lost on the OLD poses only cannot pass either.
"""
import numpy as np
import pytest

import em_ref
import fm2_cases as F


@pytest.fixture(scope="module")
def worlds():
    return {w.name: w for w in (F.rings_world(), F.corridor_world(), F.em_world())}


def _all_cases(worlds):
    return [(w, name) for w in worlds.values() for name in w.plans]


def test_c1_counts(worlds):
    rings, corridor = worlds["rings"], worlds["corridor"]
    assert set(F.RING_NM) == set(rings.plans)
    for name, nm in F.RING_NM.items():
        ref = rings.ref(name)
        e, plan = rings.plans[name]
        assert ref["nm"] == nm, name
        if name != "walked_blind":
            assert ref["n_meas"] == [F.RING_SIZES[e]] * len(plan), name
    assert rings.sims[0].num_poses() == 1 and all(s.num_poses() == 1 + len(F.RING_WALK) for s in rings.sims[1:])
    assert [s.num_landmarks() for s in rings.sims] == F.RING_SIZES  # nobody ever saw another ring
    # the named strides: 16 | 17 (T assembly), 32 | 33 and 64 | 65 | 66 (the per-pose pass), 128 | 130 (Gauss-Jordan), 256 (the cap)
    assert {16, 17, 32, 33, 64, 65, 66, 96, 128, 130, 160, 256} <= set(F.RING_NM.values())
    e, plan = F.RING_OVERFLOW
    assert F.reference(rings.sims[e], plan)["nm"] == 288
    # the corridor: more landmarks than one pass of the compaction holds, sighted ones beyond it, a plan that re-sights the first
    sim = corridor.sims[0]
    assert sim.num_landmarks() > 256 and sim.num_poses() == 1 + len(F.CORRIDOR_WALK)
    assert 3 * sim.num_poses() + 2 * sim.num_landmarks() < 700
    seen = {name: [p[1] for p in F.predicted_pairs(sim, corridor.plans[name][1])[0] if p[4]] for name in ("corridor_end", "corridor_back")}
    for name, slots in seen.items():
        nm = corridor.ref(name)["nm"]
        assert nm == len(slots) and 128 < nm <= F.MAX_MEAS, (name, nm)
        assert max(slots) >= 256, name
    assert min(seen["corridor_back"]) < 32 and max(corridor.ref("corridor_back")["n_meas"]) > 128
    assert F.reference(sim, F.CORRIDOR_OVERFLOW[1])["nm"] > F.MAX_MEAS
    for name in worlds["em_cases"].plans:
        assert (name == "em_K0" and worlds["em_cases"].ref(name)["nm"] == 0) or 0 < worlds["em_cases"].ref(name)["nm"] <= 16, name


def test_c2_no_case_sits_on_a_gate(worlds):
    worst = np.inf
    cases = [(w.sims[e], plan, name) for w in worlds.values() for name, (e, plan) in w.plans.items()]
    cases += [(worlds["rings"].sims[F.RING_OVERFLOW[0]], F.RING_OVERFLOW[1], "ring overflow"),
              (worlds["corridor"].sims[0], F.CORRIDOR_OVERFLOW[1], "corridor overflow")]
    for sim, plan, name in cases:
        if not plan:
            continue
        margin = F.predicted_pairs(sim, plan)[1]
        worst = min(worst, margin)
        assert margin > 1e-6, "%s sits on a knife edge (%.3e): choose another plan" % (name, margin)
    print("smallest gate margin %.3e" % worst)


def test_c2_the_em_cost_cases_have_margins_too(worlds):
    """The cases that tests/test_gpu_fm2.py hands to drlgx_em_cost: every gate, determinant and probability threshold of the leaf
    evaluation is decided by more than 1e-9, as tests/test_gpu_em.py requires of its own."""
    for wname, name in F.EM_COST_CASES:
        w = worlds[wname]
        e, plan = w.plans[name]
        margins = em_ref.em_cost(w.sims[e], plan, 0, cov=w.ref(name)["cov"])[3]
        print("%s: %s" % (name, margins))
        assert min(margins.values()) > 1e-9, name


def test_c3_a_dropped_update_term_would_fail(worlds):
    parity = {}
    for w, name in _all_cases(worlds):
        ref = w.ref(name)
        if ref["nm"] == 0:
            assert np.array_equal(ref["cov"], ref["base"]), name
            continue
        every, old = F.sensitivity(ref)
        print("%-14s nm %3d  update term / tolerance: all blocks %.2e, old poses %.2e" % (name, ref["nm"], every, old))
        assert every > 100.0, "%s is no parity case: the update term is %.1f x the tolerance" % (name, every)
        parity.setdefault("corridor" if w.name == "corridor" else F.band_of(ref["nm"]), []).append(name)
        if not name.startswith("fresh"):  # the plan closes a loop: the old poses alone carry the case
            assert old > 100.0, (name, old)
    print(parity)
    for band in [b[0] for b in F.BANDS] + ["corridor"]:
        assert parity.get(band), "no parity case in band %s" % band
    assert set(F.PARITY_CASES) == {n for names in parity.values() for n in names}


def test_c4_the_restatements_own_spread(worlds):
    """The figures of fm2_cases.C4_DELTA_SPREAD (and of the table above) are what is measured: round-off, so reproduced to its
    order of magnitude - within a factor of 3 - and not to the digit."""
    seen = set()
    for w, name in _all_cases(worlds):
        ref = w.ref(name)
        if ref["nm"] == 0:
            continue
        e, plan = w.plans[name]
        alt = F.reference_information_form(w.sims[e], plan)
        d_cov, d_delta = np.abs(alt["cov"] - ref["cov"]).max(), np.abs(alt["delta"] - ref["delta"]).max()
        rel = d_delta / np.abs(ref["delta"]).max()
        print("%-14s nm %3d  max |S'1 - S'2| %.2e  max |D1 - D2| %.2e  relative to max |D| %.2e  (recorded %.2e)"
              % (name, ref["nm"], d_cov, d_delta, rel, F.C4_DELTA_SPREAD[name]))
        assert rel <= 3 * F.C4_DELTA_SPREAD[name], name
        # the two evaluations share nothing but the factors: at the project's tolerance they are the same covariances
        np.testing.assert_allclose(alt["cov"], ref["cov"], rtol=F.SIGMA_RTOL * 1e-2, atol=F.SIGMA_ATOL * 1e-2, err_msg=name)
        seen.add(name)
    assert seen == set(F.C4_DELTA_SPREAD)
    # C3 for the update term's own bound: dropping the term is an error of 1 relative to max |Delta|
    assert 100 * 10 * max(F.C4_DELTA_SPREAD.values()) < 1.0


def test_information_form_prior_is_the_oracles(worlds):
    """fm2_cases.information_matrix (assembled from the factor lists) against the oracle's own joint covariance: the second
    evaluation starts from the same belief."""
    for w in worlds.values():
        for e, sim in enumerate(w.sims):
            Sig, L, P = sim.full_covariance()
            got = F._pose_blocks(F.information_matrix(sim), L, P)
            want = np.array([Sig[2 * L + 3 * i:2 * L + 3 * i + 3, 2 * L + 3 * i:2 * L + 3 * i + 3] for i in range(P)])
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-13, err_msg="%s env %d" % (w.name, e))
