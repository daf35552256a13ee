"""CPU proof (the oracle alone, no GPU) that the world of tests/obstacle_cases.py is what it claims: the oracle's return codes are
the table's, every transition of SS2D.simulate's obstacle latch occurs, and no flag hangs on a rounding."""
import math

import numpy as np

import obstacle_cases as OC
from oracle import oracle as O


def _geometry(w, ref, s, e):
    """(true distance, true bearing) of every landmark from env e's ground-truth pose after step s."""
    x, y, th = ref["veh"][s, e]
    dx, dy = w.fixed[:, 0] - x, w.fixed[:, 1] - y
    return np.hypot(dx, dy), np.arctan2(-math.sin(th) * dx + math.cos(th) * dy, math.cos(th) * dx + math.sin(th) * dy)


def test_world_shape():
    w = OC.world()
    assert w.n <= 8 and OC.N_STEPS <= 12
    assert all(len(s) == OC.N_STEPS == len(c) for s, c in zip(OC.SCRIPTS, OC.CODES))
    assert list(w.order) == list(w.make_sims()[0].ground_truth()[2])


def test_oracle_codes_are_the_table():
    ref = OC.reference()
    want = np.array([[int(c[s]) for c in OC.CODES] for s in range(OC.N_STEPS)])
    np.testing.assert_array_equal(ref["codes"], want)
    flagged = float((ref["codes"] == 2).mean())
    assert 0.25 <= flagged <= 0.75, flagged


def test_no_flag_hangs_on_a_rounding():
    """Every landmark's true distance, at every step of every env, is at least MARGIN from safe_distance; a landmark in range is at
    least 10 degrees from the bearing gate and 0.3 m from both range gates; no landmark of another env is ever in range."""
    w, ref = OC.world(), OC.reference()
    cfg = w.oracle_config()
    for s in range(OC.N_STEPS):
        for e in range(w.n):
            d, b = _geometry(w, ref, s, e)
            assert np.abs(d - OC.SAFE).min() >= OC.MARGIN, (s, e)
            inr = d < cfg.max_range + 1.0
            assert set(np.nonzero(inr)[0]) <= set(w.keys[e]), (s, e)
            assert np.abs(np.abs(b[inr]) - cfg.max_bearing).min() >= math.radians(10.0), (s, e)
            assert (d[inr] > cfg.min_range + 0.3).all() and (d[inr] < cfg.max_range - 0.3).all(), (s, e)


def _near_visible(w, ref, s, e):
    """Keys that pass the gates (by 10 degrees and more, see above) within safe_distance of env e after step s."""
    cfg = w.oracle_config()
    d, b = _geometry(w, ref, s, e)
    return [int(k) for k in np.nonzero((d < OC.SAFE) & (np.abs(b) < cfg.max_bearing))[0]]


def test_every_transition_occurs():
    w, ref = OC.world(), OC.reference()
    codes, cleared = ref["codes"], ref["cleared"]
    A, B, C, D, E, F = range(6)
    known = lambda s, e: set(int(k) for k in ref["states"][s][e].slot_keys())  # noqa: E731  (after step s)
    # clear -> hit; the latch held over a known landmark; re-armed
    assert codes[0, A] == 2 and cleared[0, A] == 0
    assert codes[1, A] == 0 and _near_visible(w, ref, 1, A) and set(_near_visible(w, ref, 1, A)) <= known(0, A) and cleared[1, A] == 1
    assert codes[2, A] == 2 and set(_near_visible(w, ref, 2, A)) <= known(1, A)
    # hit -> hit on a new landmark, first sighted in the very step it is too close, with the latch down
    assert codes[0, B] == 2 and codes[1, B] == 2 and cleared[0, B] == 0
    new = set(_near_visible(w, ref, 1, B)) - known(0, B)
    assert len(new) == 1 and new <= known(1, B)
    # a close landmark outside the bearing gate
    for s in range(3):
        d, b = _geometry(w, ref, s, C)
        close = np.nonzero(d < OC.SAFE)[0]
        assert len(close) == 1 and abs(b[close[0]]) > math.radians(OC.FOV_DEG + 50) and codes[s, C] == 0 and not _near_visible(w, ref, s, C)
    assert codes[3, C] == 2
    # the hit's place in the in-range list: 65 landmarks before it, the only near one
    cfg = w.oracle_config()
    for s in (0, 2, 4):
        d, _ = _geometry(w, ref, s, D)
        inr = [int(k) for k in w.order if d[k] < cfg.max_range]
        assert len(inr) >= 65 and _near_visible(w, ref, s, D) == [w.near_key_D] and inr.index(w.near_key_D) >= 64 and codes[s, D] == 2
    # a rejected odometry between two flagged steps; it leaves the latch alone
    assert list(codes[:3, E]) == [2, 1, 2] and list(cleared[:3, E]) == [0, 0, 0]
    assert list(codes[:4, F]) == [2, 1, 0, 2] and list(cleared[:4, F]) == [0, 0, 1, 0]
    assert set(_near_visible(w, ref, 2, F)) <= known(1, F) and _near_visible(w, ref, 2, F)


def test_safe_distance_zero_never_flags():
    w, ref = OC.world(), OC.reference()
    ocfg = w.oracle_config(safe_distance=0.0)
    sims = [O.OracleSim(ocfg, e, e, start=tuple(w.starts[e]), fixed_landmarks=w.fixed) for e in range(w.n)]
    for s in range(OC.N_STEPS):
        for e, sim in enumerate(sims):
            assert sim.simulate(ref["actions"][s, e]) == (1 if OC.SCRIPTS[e][s] == "R" else 0)
    for e, sim in enumerate(sims):  # the flag observes: the same beliefs either way
        np.testing.assert_array_equal(sim.poses()[0], ref["states"][-1][e].poses()[0])
