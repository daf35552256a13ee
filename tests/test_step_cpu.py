"""CPU checks, with the oracle alone, that the worlds of tests/step_cases.py are what they claim - before tests/test_gpu_step_edges.py
relies on them on the device:

  C1  for every environment and step the oracle's n_in (ground-truth landmarks closer than max_range), nf (factors appended), n_re
      and nn equal the table World.expected_counts; first sightings grow L by exactly nn;
  C2  no true or measured range / bearing lies within 1e-6 of a gate, and no environment ever has another ring's landmark within
      max_range + 1 m;
  C3  every re-observed landmark's 2 x 2 information block moves, from one oracle state to the next, by at least 1000 x the
      tolerance the GPU test applies to it (rtol 1e-7 / atol 1e-6): a dropped landmark of a batch would show;
  C4  at the 10th updates of the long script no |delta| reaches 0.1: no update relinearises, so every update but the reset's, the
      nf > 64 and the nn > 12 ones is expected on the incremental path - the counts inc_stats is compared with;
  C5  the form table FORMS is what the restated plan arithmetic (step_cases.inc_form) gives.

Measured here (printed with -s): smallest gate margin 0.22 (metres or radians, whichever is smaller; a measured range of a gate
landmark), foreign landmarks at least 1.27 m beyond max_range, smallest C3 ratio 1.76e3 (the long scripts; 1.2e5 in the short ones),
largest |delta| at a 10th update 0.070.
"""
import math

import numpy as np
import pytest

import step_cases as S

_cache = {}


def walk(world, script):
    """The oracles of a world stepped through a script, once: per (step + 1, environment) the observed counts, the margins, the
    C3 ratio and whether the update relinearised."""
    key = (world.name, script)
    if key in _cache:
        return _cache[key]
    cfg = world.oracle_config()
    sims = world.make_sims()
    out = dict(counts=[], margin_gate=math.inf, margin_foreign=math.inf, ratio=math.inf, relin=[], delta10=0.0, grew=[])
    own = [set(world.ring_keys[e]) | set(world.gate_keys[e]) for e in range(world.n)]

    def observe(e, sim, M0, L0, before):
        veh, lms, _ = sim.ground_truth()
        d = np.hypot(lms[:, 0] - veh[0], lms[:, 1] - veh[1])
        c, s = math.cos(veh[2]), math.sin(veh[2])
        dx, dy = lms[:, 0] - veh[0], lms[:, 1] - veh[1]
        b = np.arctan2(-s * dx + c * dy, c * dx + s * dy)
        mine = np.array(sorted(own[e]))
        foreign = np.setdiff1d(np.arange(len(lms)), mine)
        if len(foreign):
            out["margin_foreign"] = min(out["margin_foreign"], float(d[foreign].min() - cfg.max_range))
        p, k, mb, mr = sim.factors()
        inr = d < cfg.max_range
        g = min(np.abs(d - cfg.max_range).min(), np.abs(d[inr] - cfg.min_range).min(), np.abs(b[inr] - cfg.max_bearing).min(),
                np.abs(b[inr] - cfg.min_bearing).min())
        if len(mb) > M0:
            g = min(g, np.abs(mr[M0:] - cfg.max_range).min(), np.abs(mr[M0:] - cfg.min_range).min(),
                    np.abs(mb[M0:] - cfg.max_bearing).min(), np.abs(mb[M0:] - cfg.min_bearing).min())
        out["margin_gate"] = min(out["margin_gate"], float(g))
        nf, nn = len(p) - M0, sim.num_landmarks() - L0
        assert len(set(k[M0:])) == nf and set(k[M0:]) <= own[e], "a landmark twice, or another ring's"
        if before is not None:
            k0, _, i0 = before
            k1, _, i1 = sim.landmarks()
            at0, at1 = {int(x): j for j, x in enumerate(k0)}, {int(x): j for j, x in enumerate(k1)}
            for key_ in k[M0:]:
                if int(key_) in at0:
                    a, bb = i0[at0[int(key_)]], i1[at1[int(key_)]]
                    out["ratio"] = min(out["ratio"], float(np.abs(bb - a).max() / (1e-7 * np.abs(bb) + 1e-6).max()))
        return (int(inr.sum()), nf, nf - nn, nn)

    out["counts"].append([observe(e, sim, 0, 0, None) for e, sim in enumerate(sims)])
    for s, kind in enumerate(script):
        acts = world.actions(sims, kind, s)
        row, rl = [], []
        for e, sim in enumerate(sims):
            r, mx = S.relinearises(sim)
            if (s + 2) % 10 == 0:
                out["delta10"] = max(out["delta10"], mx)
            rl.append(r)
            M0, L0, before = len(sim.factors()[0]), sim.num_landmarks(), sim.landmarks()
            assert sim.simulate(acts[e]) == 0
            row.append(observe(e, sim, M0, L0, before))
        out["counts"].append(row)
        out["relin"].append(rl)
    out["sims"] = sims
    _cache[key] = out
    return out


_INC = [(w, s) for w in ("small", "large") for s in ("short", "long")]


@pytest.mark.parametrize("wname,sname", _INC)
def test_counts_margins_sensitivity_and_deltas(wname, sname):
    world, script = S.WORLDS[wname](), S.SCRIPTS[sname]
    got = walk(world, script)
    want = world.expected_counts(script)
    print("\n%s / %s: (n_in, nf, n_re, nn) per ring %s" % (wname, sname, [r for r, _ in world.rings]))
    for s in sorted({-1, 0, 1} | {t for t, k in enumerate(script) if k in "gb"} | ({51, 52} if sname == "long" else set())):
        print("  step %2d (%s): %s" % (s, script[s] if s >= 0 else "reset", got["counts"][s + 1]))
    assert got["counts"] == want                                                      # C1
    print("  gate margin %.3e, foreign landmarks beyond max_range by %.2f m, smallest C3 ratio %.3e, max |delta| at a 10th update %.3f,"
          " relinearising updates per environment %s" % (got["margin_gate"], got["margin_foreign"], got["ratio"], got["delta10"],
                                                         np.sum(got["relin"], axis=0).tolist()))
    assert got["margin_gate"] > 1e-6 and got["margin_foreign"] > S.MAX_RANGE_MARGIN   # C2
    assert got["ratio"] >= 1000.0                                                     # C3
    assert got["delta10"] < 0.1 and not np.any(got["relin"])                          # C4: zero relinearising updates expected
    for sim, (size, gate) in zip(got["sims"], world.rings):
        assert sim.num_landmarks() == size + gate and sim.num_poses() == len(script) + 1
    # every listed count is reached on the incremental worlds' k_inc edges, in this script
    flat = [c for row in got["counts"][1:] for c in row]
    if wname == "small":
        assert {c[2] for c in flat} >= {8, 9, 16, 17, 24, 25, 32, 33} and {c[3] for c in flat} >= {1, 12, 13}
    else:
        assert {c[2] for c in flat} >= {48, 52, 63, 64, 65} and (64, 64, 52, 12) in flat and (65, 65, 64, 1) in flat
        assert (64, 64, 64, 0) in flat and all(c[1] == 65 for row in got["counts"] for c in row[4:])
    paths = [[S.expected_path(c, s + 2, got["relin"][s][e]) for e, c in enumerate(row)] for s, row in enumerate(got["counts"][1:])]
    assert all(p == "full" for p in np.array(paths)[:, -1]) if wname == "large" else True   # the ring of 65: never incremental


@pytest.mark.parametrize("world", S.sim_worlds(), ids=lambda w: w.name)
def test_sim_worlds_reach_their_counts(world):
    got = walk(world, S.SIM_SCRIPT + "j")
    want = world.expected_counts(S.SIM_SCRIPT + "j")
    print("\n%s: n_in per environment %s, gate margin %.3e, foreign %.2f m" % (world.name, [c[0] for c in got["counts"][1]], got["margin_gate"],
                                                                             got["margin_foreign"]))
    assert got["counts"] == want and [c[0] for c in got["counts"][1]] == S.SIM_N_IN[world.name]
    assert got["margin_gate"] > 1e-6 and got["margin_foreign"] > S.MAX_RANGE_MARGIN
    assert (world.num_landmarks <= 128) == world.name.startswith("pre")


def test_sim_worlds_cover_the_listed_counts():
    pre = {n for w in S.sim_worlds() if w.num_landmarks <= 128 for n, _ in w.rings}
    loop = {n for w in S.sim_worlds() if w.num_landmarks > 128 for n, _ in w.rings}
    assert pre >= {63, 64, 65, 128} and loop >= {64, 65, 128, 129, 130}


def test_capacity_world():
    world = S.capacity_world()
    got = walk(world, "jgb")
    assert got["counts"] == world.expected_counts("jgb") and got["counts"][2][0] == (77, 77, 65, 12)
    assert got["margin_gate"] > 1e-6 and got["margin_foreign"] > S.MAX_RANGE_MARGIN


def test_form_table_is_the_plan_arithmetic():
    for wname, make in S.WORLDS.items():
        for sname, script in S.SCRIPTS.items():
            assert S.FORMS[wname][sname] == S.form_table(make(), script), (wname, sname)
    forms = {f for w in S.FORMS.values() for t in w.values() for f in t.values()}
    print("\nforms reached: %s" % sorted(forms))
    # the panel in LDS and in HBM / L2, the wide two-walk form, and the streamed form with 3 and 4 tiles in its first walk and
    # 1, 2, 3 and 4 in its second (the narrow forms, first walks of one and two tiles and a plan that misses the LDS are reached by
    # the worlds of tests/inc_form_cases.py, not by these: here the second half of Y fits the LDS everywhere)
    assert forms >= {"lds wide", "two-walk wide", "streamed 3", "streamed 4", "streamed 4+1", "streamed 4+2", "streamed 4+3", "streamed 4+4"}
    # the fallback edges, one case on either side (csrc/k_inc.hip: INF = 64, INEW = 12)
    assert S.expected_path((64, 64, 52, 12), 5, False) == "inc" and S.expected_path((65, 65, 64, 1), 5, False) == "full"
    assert S.expected_path((29, 29, 17, 12), 5, False) == "inc" and S.expected_path((46, 46, 33, 13), 5, False) == "full"
