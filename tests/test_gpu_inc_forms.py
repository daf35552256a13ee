"""GPU tests (run with -m gpu on an MI355X) of the incremental belief update (csrc/k_inc.hip) in the forms only the worlds of
tests/inc_form_cases.py reach (tests/test_inc_form_cases_cpu.py proves on the CPU that they do), and of the host's
drlgx_debug_inc_form - the plan of csrc/inc_carve.h - against the restatement tests/step_cases.py::inc_form.

Per world, three sides by side: the incremental engine, an engine created under DRLGX_INCREMENTAL=0, the oracle.  At the check step
and the two steps behind it, per case (= environment):
  1. drlgx_debug_inc_form, fed from eng.counts and eng.panel taken before the step and the launch's pose bound, is the claimed cell;
  2. the environment is stepped alone: inc_stats advances by (1, 0), by (0, 1) in the cell whose plan misses the LDS;
  3. incremental engine against full-solve engine at _compare_engines' tolerances (tests/test_gpu_step_edges.py), unchanged;
  4. both against the oracle by compare_state (tests/test_gpu_belief.py);
  5. the covariance panel against the oracle's covariance: rtol 1e-7 + atol 1e-7 x the largest diagonal entry.
Tolerances: the project's parity bar, unchanged; the virtual map of the pose-chain worlds at 1e-6, as in the long scripts of
test_incremental_update_at_its_batch_edges.  Each world prints its cells, the measured gaps as shares of the tolerance and its wall time.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import inc_form_cases as F  # noqa: E402
import lazy_panel_cases as LP  # noqa: E402
import step_cases as S  # noqa: E402
from test_gpu_arrow_forms import _panel_against_oracle  # noqa: E402
from test_gpu_belief import compare_state  # noqa: E402
from test_gpu_step_edges import _assert_bits, _compare_engines, _dump, _engine, _step  # noqa: E402
from test_inc_form_cases_cpu import calls_before  # noqa: E402

CASE_OF = {(c[1], c[2]): c for c in F.CASES}


# ------------------------------------------------------------------------------------- 1. the restatement against the host function
def _same(P, L0, n_re, LG, P_max, L_max, pc):
    got = F.host_form(P, L0, n_re, pc, P_max, L_max, LG)[0]
    want = S.inc_form(P, L0, n_re, LG, P_max, L_max, pc=pc)
    assert got == want, "P %d L0 %d n_re %d pc %d, capacities (%d, %d), LG %d: inc_carve.h %s, step_cases.inc_form %s" % (
        P, L0, n_re, pc, P_max, L_max, LG, got, want)
    return got


def test_restated_plan_equals_the_host_function():
    """step_cases.inc_form against drlgx_debug_inc_form over the tables of step_cases.py and lazy_panel_cases.py, every case of
    inc_form_cases.py, and a grid of (P, L0, n_re, pose bound) at the capacities of all of those worlds."""
    t0 = time.time()
    seen = set()
    for wname, make in S.WORLDS.items():
        world = make()
        for sname, script in S.SCRIPTS.items():
            counts = world.expected_counts(script)
            for (size, s), form in S.FORMS[wname][sname].items():
                e = [r for r, _ in world.rings].index(size)
                gate = world.rings[e][1]
                L0 = size + (gate if any(script[t] == "g" for t in range(s)) else 0)
                assert _same(s + 2, L0, counts[s + 1][e][2], world.num_landmarks, world.caps["max_poses"], world.caps["max_landmarks"], s + 2) == form
                seen.add(form)
    lp_worlds = {"inplace": LP.inplace_world(), "small": LP.small_world()}
    for (wname, ring, P), form in LP.FORMS.items():
        world = lp_worlds[wname]
        e = [r for r, _ in world.rings].index(ring)
        L0 = ring + (world.rings[e][1] if wname == "inplace" and P >= 4 else 0)
        got = _same(P, L0, ring, world.num_landmarks, world.caps["max_poses"], world.caps["max_landmarks"], P)
        assert got == LP.form(world, e, P, ring, wname == "inplace" and P >= 4)
        assert got == form, (wname, ring, P, got)
    grid_worlds = F.worlds() + [S.small_world(), S.large_world(), LP.inplace_world(), LP.chain_world()]
    for name, wname, e, cell in F.CASES:
        world = {w.name: w for w in F.worlds()}[wname]
        P, L0, n_re, _ = world.expected(e, world.check_step)
        assert _same(P, L0, n_re, world.num_landmarks, world.caps["max_poses"], world.caps["max_landmarks"], P) == cell
    n = 0
    for world in grid_worlds:
        P_max, L_max, LG = world.caps["max_poses"], world.caps["max_landmarks"], world.num_landmarks
        poses = sorted({p for p in (2, 3, 4, 6, 12, 37, 52, 53, 54, 55, 56, 58, 60, 64, 100, 119, 121, 128) if p <= P_max} | {P_max})
        lms = sorted(set(range(1, min(L_max, 48) + 1)) | set(range(48, L_max + 1, 7)) | {L_max - 1, L_max})
        for P in poses:
            for L0 in lms:
                for n_re in (0, 1, 8, 9, 16, 17, 24, 25, 32, 33, 64):
                    if n_re <= L0:
                        for pc in {P, P_max}:
                            seen.add(_same(P, L0, n_re, LG, P_max, L_max, pc))
                            n += 1
    print("\n%d grid points in %.2f s; forms seen: %s" % (n, time.time() - t0, sorted(seen)))
    assert seen >= {c[3] for c in F.CASES} | {"lds wide", "two-walk wide", "streamed 4+4"}
    # arguments out of range are refused
    from drl_graph_exploration_amd import _lib
    import ctypes as C
    out = (C.c_int32 * 14)()
    L = _lib.lib()
    assert L.drlgx_debug_inc_form(1, 3, 1, 1, 8, 8, 8, S.LDS_BUDGET, out) != 0 and L.drlgx_debug_inc_form(9, 3, 1, 8, 8, 8, 8, S.LDS_BUDGET, out) != 0
    assert L.drlgx_debug_inc_form(4, 9, 1, 4, 8, 8, 8, S.LDS_BUDGET, out) != 0 and L.drlgx_debug_inc_form(4, 3, 4, 4, 8, 8, 8, S.LDS_BUDGET, out) != 0
    assert L.drlgx_debug_inc_form(4, 3, 1, 4, 8, 8, 8, S.LDS_BUDGET + 1, out) != 0 and L.drlgx_debug_inc_form(4, 3, 1, 4, 8, 8, 8, S.LDS_BUDGET, None) != 0


# --------------------------------------------------------------------------- 2. every form against the full solve and the oracle
def _share(a, b, rtol, atol):
    """largest |a - b| as a share of atol + rtol |b| (assert_allclose's bound)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max()) if a.size else 0.0


def _gaps(x, y):
    """(estimates, information blocks): the largest share of _compare_engines' / compare_state's tolerance between two sides, each
    (pose estimates, pose information, landmark estimates, landmark information)."""
    return (max(_share(x[0], y[0], 0.0, 1e-9), _share(x[2], y[2], 0.0, 1e-9)), max(_share(x[1], y[1], 1e-7, 1e-6), _share(x[3], y[3], 1e-7, 1e-6)))


def _sides(eng, ref, sim, i):
    xyt, info = eng.poses(i)
    _, xy, linfo = eng.landmarks(i)
    rxyt, rinfo = ref.poses(i)
    _, rxy, rlinfo = ref.landmarks(i)
    oxyt, oinfo = sim.poses()
    _, oxy, olinfo = sim.landmarks()
    return (xyt, info, xy, linfo), (rxyt, rinfo, rxy, rlinfo), (oxyt, oinfo, oxy, olinfo)


@pytest.mark.parametrize("world", F.worlds(), ids=lambda w: w.name)
def test_every_form_against_full_solve_and_oracle(world, monkeypatch):
    t0 = time.time()
    run = F.walk(world)
    t_oracle = time.time() - t0
    dense = not world.name.startswith("chain")
    eng = _engine(world)
    monkeypatch.setenv("DRLGX_INCREMENTAL", "0")
    ref = _engine(world)
    monkeypatch.delenv("DRLGX_INCREMENTAL")
    assert ref.inc_stats() == (-1, -1) and eng.inc_stats() == (0, world.n)
    P_max, L_max, LG = world.caps["max_poses"], world.caps["max_landmarks"], world.num_landmarks
    calls = 0
    try:
        for s in range(len(world.script)):
            acts = run["actions"][s]
            if s < world.check_step:
                _step([eng, ref], acts)
                calls += 1
                continue
            for e in range(world.n):
                name, _, _, cell = CASE_OF[(world.name, e)]
                P, L0_want, nf, n_re, nn, _, _ = run["rows"][s][e]
                # 1. the plan of the kernel's header, from the engine's own state before the step
                c0 = eng.counts(e)
                meta, _ = eng.panel(e)
                assert meta[0] == 1 and meta[1] == c0["poses"] and meta[2] == c0["landmarks"] == L0_want, (name, s, meta, c0)
                assert calls == calls_before(world, s, e)
                form, raw = F.host_form(c0["poses"] + 1, int(meta[2]), n_re, F.pose_bound(world, calls), P_max, L_max, LG)
                assert form == cell, "%s step %d: drlgx_debug_inc_form says %s %s" % (name, s, form, raw)
                if name in F.BATCHES:
                    assert raw[5] == F.BATCHES[name] and raw[6:6 + raw[5]] == [1] * raw[5], (name, raw)
                # 2. stepped alone: which path served it
                b0 = eng.inc_stats()
                _step([eng, ref], acts, only=e)
                calls += 1
                assert eng.status() == 0 and ref.status() == 0
                b1 = eng.inc_stats()
                c1 = eng.counts(e)
                assert (c1["poses"], c1["landmarks"] - c0["landmarks"], c1["factors"] - c0["factors"]) == (P, nn, nf), (name, s, c0, c1)
                assert (b1[0] - b0[0], b1[1] - b0[1]) == ((0, 1) if cell == "none" else (1, 0)), "%s step %d (%s): inc_stats %s -> %s" % (name, s, cell, b0, b1)
            for e, sim in enumerate(run["snaps"][s]):
                name, _, _, cell = CASE_OF[(world.name, e)]
                what = "%s (%s) step %d" % (name, cell, s)
                a, r, o = _sides(eng, ref, sim, e)
                print("%s: share of the tolerance (estimates, information) - incremental vs full solve %.3e %.3e, full solve vs oracle %.3e %.3e, "
                      "incremental vs oracle %.3e %.3e" % ((what,) + _gaps(a, r) + _gaps(r, o) + _gaps(a, o)))
                _compare_engines(eng, ref, e, what)                                                    # 3
                compare_state(eng, e, sim, "incremental, " + what, check_vm=dense)                     # 4
                compare_state(ref, e, sim, "full solve, " + what, check_vm=dense)
                if not dense:  # (the virtual map at 1e-6 in the long scripts)
                    prob, vinfo, tr, upd = eng.virtual_map(e)
                    oprob, ovinfo, otr, oupd = sim.virtual_map()
                    np.testing.assert_array_equal(upd, oupd)
                    np.testing.assert_allclose(prob, oprob, rtol=1e-14, err_msg=what)
                    np.testing.assert_allclose(vinfo, ovinfo, rtol=1e-6, atol=1e-9, err_msg=what)
                    np.testing.assert_allclose(tr, otr, rtol=1e-6, err_msg=what)
                _panel_against_oracle(eng, e, sim, what)                                               # 5
    finally:
        eng.close()
        ref.close()
    print("%s: %.1f s (oracle walk %.1f s)" % (world.name, time.time() - t0, t_oracle))


# ------------------------------------------------------------------------------------- 3. fused step = stage kernels, narrow forms
_NARROW = [w for w in F.worlds() if w.name in ("dense100", "dense270", "chain270a", "chain64", "chain32")]


@pytest.mark.parametrize("world", _NARROW, ids=lambda w: w.name)
def test_fused_step_equals_stage_kernels_in_the_narrow_forms(world):
    """timing_enable(2) - the three stage kernels - against the default form, bit for bit, at the check step and behind it: both
    take the same instantiation (lds / two-walk narrow; one, two and three narrow batches; streamed 1, 2, 2+1)."""
    run = F.walk(world)
    fused, staged = _engine(world), _engine(world)
    staged.timing_enable(2)
    try:
        for s in range(len(world.script)):
            before = fused.inc_stats(), staged.inc_stats()
            _step([fused, staged], run["actions"][s])
            if s < world.check_step:
                continue
            assert fused.status() == 0 and staged.status() == 0
            after = fused.inc_stats(), staged.inc_stats()
            for b, a in zip(before, after):
                assert (a[0] - b[0], a[1] - b[1]) == (world.n, 0), (s, before, after)
            for i in range(world.n):
                assert fused.counts(i) == staged.counts(i)
                _assert_bits(_dump(fused, i), _dump(staged, i), "%s env %d step %d" % (world.name, i, s))
                fm, fb = fused.panel(i)
                sm, sb = staged.panel(i)
                _assert_bits((fm, fb), (sm, sb), "%s env %d step %d: panel" % (world.name, i, s))
        tm = staged.timing_read()
        assert tm["slam"][1] == len(world.script) and tm["step"][1] == 0
    finally:
        fused.close()
        staged.close()
