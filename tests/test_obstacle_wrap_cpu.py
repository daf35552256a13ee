"""CPU proof (the oracle alone, no GPU) that the worlds of tests/obstacle_wrap_cases.py are what they claim: the return codes, the
in-range count of every step, the place of every hit in the iteration-ordered in-range list, which near landmarks are first
sightings, the margins, and that no environment sees another's landmarks."""
import math

import numpy as np
import pytest

import obstacle_wrap_cases as WC

WORLDS = {"W": (WC.world_w, WC.reference_w, WC.W_N_IN), "A": (WC.world_a, WC.reference_a, WC.A_N_IN)}


def _geometry(w, ref, s, e):
    """(true distance, true bearing) of every landmark from env e's ground-truth pose after step s."""
    x, y, th = ref["veh"][s, e]
    dx, dy = w.fixed[:, 0] - x, w.fixed[:, 1] - y
    return np.hypot(dx, dy), np.arctan2(-math.sin(th) * dx + math.cos(th) * dy, math.cos(th) * dx + math.sin(th) * dy)


def _in_range(w, ref, s, e):
    """Env e's in-range list after step s, in iteration order."""
    d, _ = _geometry(w, ref, s, e)
    return [int(k) for k in w.order if d[k] < w.oracle_config().max_range]


def _near_visible(w, ref, s, e):
    """Keys that pass the gates within safe_distance of env e after step s."""
    cfg = w.oracle_config()
    d, b = _geometry(w, ref, s, e)
    return [int(k) for k in np.nonzero((d < WC.SAFE) & (np.abs(b) < cfg.max_bearing))[0]]


def _known_before(ref, s, e):
    """The oracle's slot keys before step s."""
    return set(int(k) for k in ref["before"][s][e].slot_keys())


@pytest.mark.parametrize("name", list(WORLDS))
def test_shape_codes_and_in_range_counts(name):
    w, ref, n_in = WORLDS[name][0](), WORLDS[name][1](), WORLDS[name][2]
    assert w.n <= 8 and w.n_steps <= 8 and 129 <= w.num_landmarks <= 330
    assert all(len(s) == w.n_steps == len(c) for s, c in zip(w.scripts, w.codes))
    assert list(w.order) == list(w.make_sims()[0].ground_truth()[2])
    want = np.array([[int(c[s]) for c in w.codes] for s in range(w.n_steps)])
    np.testing.assert_array_equal(ref["codes"], want)
    for e in range(w.n):
        got = [len(_in_range(w, ref, s, e)) for s in range(w.n_steps)]
        print("world %s env %s n_in %s" % (name, w.names[e], got))
        assert got == n_in[e]
    # the capacities are the oracle's own counts (landmarks rounded up to 8, factors to 64)
    last = ref["states"][-1]
    caps = ref["caps"]
    assert caps["max_poses"] == max(s.num_poses() for s in last)
    assert 0 <= caps["max_landmarks"] - max(s.num_landmarks() for s in last) < 8
    assert 0 <= caps["max_factors"] - max(len(s.factors()[0]) for s in last) < 64


def test_flagged_share():
    codes = np.concatenate([WC.reference_w()["codes"].ravel(), WC.reference_a()["codes"].ravel()])
    flagged = float((codes == 2).mean())
    assert 0.25 <= flagged <= 0.75, flagged


def test_every_in_range_count_occurs():
    seen = set(n for row in WC.W_N_IN + WC.A_N_IN for n in row)
    assert {63, 64, 65, 128, 129} <= seen and max(seen) >= 130
    assert WC.A_N_IN == [[WC.world_a().num_landmarks] * 2]  # n_in == LG at every step


@pytest.mark.parametrize("name", list(WORLDS))
def test_no_flag_hangs_on_a_rounding(name):
    """Every landmark's true distance, at every step of every env, is at least MARGIN from safe_distance and 0.3 m from max_range;
    a landmark in range is at least 10 degrees from the bearing gate and 0.3 m from both range gates; no landmark of another env
    is ever within max_range + 1."""
    w, ref = WORLDS[name][0](), WORLDS[name][1]()
    cfg = w.oracle_config()
    for s in range(w.n_steps):
        for e in range(w.n):
            d, b = _geometry(w, ref, s, e)
            assert np.abs(d - WC.SAFE).min() >= WC.MARGIN, (s, e)
            assert np.abs(d - cfg.max_range).min() >= 0.3, (s, e)
            assert set(np.nonzero(d < cfg.max_range + 1.0)[0]) <= set(w.keys[e]), (s, e)
            inr = d < cfg.max_range
            assert np.abs(np.abs(b[inr]) - cfg.max_bearing).min() >= math.radians(10.0), (s, e)
            assert (d[inr] > cfg.min_range + 0.3).all() and (d[inr] < cfg.max_range - 0.3).all(), (s, e)


def test_world_w_hits():
    w, ref = WC.world_w(), WC.reference_w()
    codes, cleared = ref["codes"], ref["cleared"]
    X, Y, Z = range(3)
    key = lambda e, which: WC.near_key(w, e, which)  # noqa: E731
    place = lambda s, e, k: _in_range(w, ref, s, e).index(k) + 1  # noqa: E731
    # the listed places, at every step at the centre
    for (env, which), p in WC.W_PLACE.items():
        e = WC.W_NAMES.index(env)
        for s in range(w.n_steps):
            if w.scripts[e][s] in "ct":
                assert place(s, e, key(e, which)) == p, (env, which, s)
    # X, Y: step 0 the single near landmark is K (known from the reset's measure(), latch up), at place 64 of 65 - the second trip
    # holds one landmark and no hit - and 128 of 130
    for e, p, n in ((X, 64, 65), (Y, 128, 130)):
        assert _near_visible(w, ref, 0, e) == [key(e, "K")] and key(e, "K") in _known_before(ref, 0, e)
        assert codes[0, e] == 2 and place(0, e, key(e, "K")) == p and len(_in_range(w, ref, 0, e)) == n
        # step 1: N, first sighted in the very step it is too close, with the latch down, at place 65 / 129: flags
        assert cleared[0, e] == 0 and _near_visible(w, ref, 1, e) == [key(e, "N")] and key(e, "N") not in _known_before(ref, 1, e)
        assert codes[1, e] == 2 and place(1, e, key(e, "N")) == p + 1
        # step 2: the same landmark known, latch down: does not flag, re-arms; step 3: flags
        assert cleared[1, e] == 0 and _near_visible(w, ref, 2, e) == [key(e, "N")] and key(e, "N") in _known_before(ref, 2, e)
        assert codes[2, e] == 0 and cleared[2, e] == 1 and codes[3, e] == 2
        # steps 4, 5: nothing near in the gate, one pad less in range each
        assert not _near_visible(w, ref, 4, e) and not _near_visible(w, ref, 5, e)
    # Z: the hit at the last place
    assert _near_visible(w, ref, 0, Z) == [key(Z, "K")] and place(0, Z, key(Z, "K")) == 130 == len(_in_range(w, ref, 0, Z))
    assert codes[0, Z] == 2
    # step 1: K known at a place >= 129 with the latch down does not flag; N - too close, never sighted, place 129, latch DOWN at
    # step 1 and UP at step 2's start - is outside the bearing gate by 50 degrees and more and never counts
    assert cleared[0, Z] == 0 and _near_visible(w, ref, 1, Z) == [key(Z, "K")] and key(Z, "K") in _known_before(ref, 1, Z)
    assert codes[1, Z] == 0 and cleared[1, Z] == 1
    for s in range(3):
        d, b = _geometry(w, ref, s, Z)
        n = key(Z, "N")
        assert d[n] < WC.SAFE - WC.MARGIN and abs(b[n]) > math.radians(WC.OC.FOV_DEG + 50) and n not in _known_before(ref, s + 1, Z)
        assert place(s, Z, n) == 129
    # a rejected odometry between two flagged steps; it leaves the latch alone; then N new with the latch down flags
    assert list(codes[2:5, Z]) == [2, 1, 2] and list(cleared[2:5, Z]) == [0, 0, 0]
    assert _near_visible(w, ref, 4, Z) == [key(Z, "N")] and key(Z, "N") not in _known_before(ref, 4, Z)
    assert codes[5, Z] == 0 and _near_visible(w, ref, 5, Z) == [key(Z, "N")]


def test_world_a_hits_every_trip_at_once():
    w, ref = WC.world_a(), WC.reference_a()
    assert not _known_before(ref, 0, 0)  # the reset sighted nothing
    inr = _in_range(w, ref, 0, 0)
    assert len(inr) == w.num_landmarks == 131
    places = sorted(inr.index(k) + 1 for k in _near_visible(w, ref, 0, 0))
    assert places == list(WC.A_PLACES) and places[0] <= 64 < places[1] <= 128 < places[2] == 131
    assert ref["codes"][0, 0] == 2 and ref["states"][0][0].num_landmarks() == 131  # 131 first sightings in one call
    assert ref["codes"][1, 0] == 0 and not _near_visible(w, ref, 1, 0) and len(_in_range(w, ref, 1, 0)) == 131
