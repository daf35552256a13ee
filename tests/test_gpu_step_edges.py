"""GPU tests (run with -m gpu on an MI355X) of the belief step - k_sim -> k_inc / k_slam / k_slam_arrow -> k_map, fused in k_step -
where a step's factors wrap waves and batches, through the C ABI, on the listed-landmark worlds of tests/step_cases.py (whose
counts, gate margins, sensitivity and expected update paths tests/test_step_cpu.py proves on the CPU).

Tolerances: the project's parity bar, unchanged - topology, keys and flags exact, RNG-path values 1e-12,
estimates 1e-9, information blocks rtol 1e-7 / atol 1e-6, virtual-map information 1e-7 relative (1e-6 in the long scripts, as in
the 31-step incremental test), look-ahead rewards 1e-6, A/Bs of kernel form bit-equal.

Why the capacity test may run (test_capacity_is_a_status): every store of the simulator is behind a check against the instance's
own capacities.  sim_step_body returns before anything is loaded or stored when P >= P_max (flag + status only), so th_pose / d_pose
/ odo are written at index P_before < P_max.  measure() decides per trip of 64: c.L + n_new > L_max or c.M + n_ok > M_max sets the
error and returns BEFORE the trip's stores, so every landmark slot written is < L_max, every factor index < M_max, key_slot is
indexed by a ground-truth key < num_landmarks <= LG, and the LDS hand-over writes nrm[2 r], inr[r], lmbox[2 j] with r <= the lane's
own input index < n_in <= LG and j < the new landmarks of this call <= LG.  store_ctx writes counters only.  replay_step_body
appends what k_presim logged under the same two checks (its header carries the error).  inc_post's `feasible` refuses nf > 64,
nn > 12 and L > Lcap = min(L_max, L0 + 12) before it reads a list, and reads at most nf <= 64 slots; the solvers' entries
(slam_finish, arrow_body) read the counts the simulator left, which are within the capacities, and return on a rejected move.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import step_cases as S  # noqa: E402
from test_gpu_belief import compare_state  # noqa: E402
from test_gpu_em import DRLGX_E_CAPACITY  # noqa: E402


def _engine(world, n_roll=0, **caps):
    from drl_graph_exploration_amd.engine import Engine
    eng = Engine(world.engine_config(**caps), world.n, n_roll)
    eng.set_fixed_landmarks(world.fixed)
    eng.reset(np.arange(world.n), np.arange(world.n), starts=world.starts)
    assert eng.status() == 0
    return eng


def _step(engines, acts, only=None):
    for eng in engines:
        odom = torch.tensor(acts, dtype=torch.float64, device=eng.device)
        active = None
        if only is not None:
            m = np.zeros(len(acts), dtype=np.uint8)
            m[only] = 1
            active = torch.tensor(m, device=eng.device)
        eng.step(odom, active)


def _dump(eng, i, vm=True):
    return eng.poses(i) + eng.landmarks(i) + eng.factors(i) + eng.ground_truth(i) + (eng.virtual_map(i) if vm else ())


def _assert_bits(a, b, msg):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg=msg)


def _new_factors(eng, i):
    """(keys, bearing, range) of the factors on instance i's newest pose, in factor order."""
    p, k, b, r = eng.factors(i)
    sel = p == eng.counts(i)["poses"] - 1
    return k[sel], b[sel], r[sel]


# ---------------------------------------------------------------------------------------------- 1. simulator parity at the wraps
@pytest.mark.parametrize("world", S.sim_worlds(), ids=lambda w: w.name)
def test_simulator_parity_at_the_wraps(world):
    """compare_state after the reset and after every step (three, and one further step: both random streams and the saved-variate
    flags sit where the reference's do); the staged interface exports, bit for bit, the factors the fused step appends."""
    sims = world.make_sims()
    from drl_graph_exploration_amd.engine import Engine
    eng = _engine(world)
    stg = Engine(world.engine_config(), world.n, 0)
    stg.set_fixed_landmarks(world.fixed)
    stg.stage_reset(np.arange(world.n), np.arange(world.n), world.starts)
    k, br, c = stg.stage_measure()
    stg.stage_add_measurements(k, br, c)
    stg.stage_optimize()
    want = world.expected_counts(S.SIM_SCRIPT + "j")

    def check(step):
        kh, bh, ch = k.cpu().numpy(), br.cpu().numpy(), c.cpu().numpy()
        for i, sim in enumerate(sims):
            name = "%s env %d step %d" % (world.name, i, step)
            compare_state(eng, i, sim, name, check_vm=step >= 0)
            fk, fb, fr = _new_factors(eng, i)
            assert len(fk) == want[step + 1][i][1] == ch[i], name
            np.testing.assert_array_equal(kh[i, :ch[i]], fk, err_msg=name)
            _assert_bits((bh[i, :ch[i], 0], bh[i, :ch[i], 1]), (fb, fr), name)
            assert stg.counts(i) == eng.counts(i), name

    check(-1)
    for s, kind in enumerate(S.SIM_SCRIPT + "j"):
        acts = world.actions(sims, kind, s)
        _step([eng], acts)
        stg.stage_move(torch.tensor(acts, dtype=torch.float64, device=stg.device))
        stg.stage_measure()  # SS2D.simulate's first measure(): only the sensor stream advances
        k, br, c = stg.stage_measure()
        stg.stage_add_measurements(k, br, c)
        stg.stage_optimize()
        for sim, a in zip(sims, acts):
            sim.simulate(a)
        assert eng.status() == 0 and stg.status() == 0
        check(s)
    eng.close()
    stg.close()


# ------------------------------------------------------------------------------------------------ 2. fused step = stage kernels
_AB = [(w.name, w, S.SIM_SCRIPT + "j") for w in S.sim_worlds()] + [("%s_%s" % (w, s), S.WORLDS[w](), S.SCRIPTS[s]) for w in S.WORLDS for s in S.SCRIPTS]


@pytest.mark.parametrize("name,world,script", _AB, ids=[a[0] for a in _AB])
def test_fused_step_equals_stage_kernels_at_these_counts(name, world, script):
    """timing_enable(2) - the three stage kernels - against the default form: the state dumps bit for bit, step after step (the
    virtual map at the steps of LONG_CHECKS in the long scripts).  Includes the in-place nrm / inr hand-over with more than 64 factors."""
    sims = world.make_sims()
    fused, staged = _engine(world), _engine(world)
    staged.timing_enable(2)
    for s, kind in enumerate(script):
        acts = world.actions(sims, kind, s)
        _step([fused, staged], acts)
        for sim, a in zip(sims, acts):
            sim.simulate(a)
        vm = len(script) < 10 or s in S.LONG_CHECKS
        for i in range(world.n):
            assert fused.counts(i) == staged.counts(i)
            _assert_bits(_dump(fused, i, vm), _dump(staged, i, vm), "%s env %d step %d" % (name, i, s))
    assert fused.status() == 0 and staged.status() == 0
    tm = staged.timing_read()
    assert tm["slam"][1] == len(script) and tm["step"][1] == 0
    fused.close()
    staged.close()


# ------------------------------------------------------------------------------------- 3. incremental update at its batch edges
def _compare_engines(eng, ref, i, name):
    xyt, info = eng.poses(i)
    rxyt, rinfo = ref.poses(i)
    np.testing.assert_allclose(xyt, rxyt, atol=1e-9, err_msg=name)
    np.testing.assert_allclose(info, rinfo, rtol=1e-7, atol=1e-6, err_msg=name)
    k, xy, linfo = eng.landmarks(i)
    rk, rxy, rlinfo = ref.landmarks(i)
    np.testing.assert_array_equal(k, rk)
    np.testing.assert_allclose(xy, rxy, atol=1e-9, err_msg=name)
    np.testing.assert_allclose(linfo, rlinfo, rtol=1e-7, atol=1e-6, err_msg=name)
    np.testing.assert_array_equal(eng.virtual_map(i)[3], ref.virtual_map(i)[3])


_INC = [(w, s) for w in S.WORLDS for s in S.SCRIPTS]


@pytest.mark.parametrize("wname,sname", _INC, ids=["%s_%s" % c for c in _INC])
def test_incremental_update_at_its_batch_edges(wname, sname, monkeypatch):
    """The incremental engine, an engine created under DRLGX_INCREMENTAL=0 and the oracle side by side: every step of the short
    script, the steps of LONG_CHECKS of the long one.  At the boundary steps (all of the short script, LONG_SOLO of the long one) the
    environments are stepped one at a time, so that the delta of inc_stats says which path served WHICH environment: nf = 64 with
    nn = 12 incrementally, nf = 65, nn = 13 and the ring of 65 by a full solve, every other update incrementally (no update of
    these scripts relinearises: test_step_cpu.py C4)."""
    world, script = S.WORLDS[wname](), S.SCRIPTS[sname]
    short = sname == "short"
    sims = world.make_sims()
    eng = _engine(world)
    monkeypatch.setenv("DRLGX_INCREMENTAL", "0")
    ref = _engine(world)
    monkeypatch.delenv("DRLGX_INCREMENTAL")
    assert ref.inc_stats() == (-1, -1) and eng.inc_stats() == (0, world.n)
    counts = world.expected_counts(script)
    seen_paths = set()
    for s, kind in enumerate(script):
        acts = world.actions(sims, kind, s)
        want = [S.expected_path(counts[s + 1][e], s + 2, S.relinearises(sims[e])[0]) for e in range(world.n)]
        before = eng.inc_stats()
        if short or s in S.LONG_SOLO:
            for e in range(world.n):
                b0 = eng.inc_stats()
                _step([eng, ref], acts, only=e)
                assert eng.status() == 0 and ref.status() == 0
                b1 = eng.inc_stats()
                got = "inc" if (b1[0] - b0[0], b1[1] - b0[1]) == (1, 0) else "full" if (b1[0] - b0[0], b1[1] - b0[1]) == (0, 1) else None
                assert got == want[e], "%s/%s step %d ring %d %s: served by %s (%s -> %s), expected %s" % (
                    wname, sname, s, world.rings[e][0], counts[s + 1][e], got, b0, b1, want[e])
                seen_paths.add((counts[s + 1][e][1] > S.INF, counts[s + 1][e][3] > S.INEW, got))
        else:
            _step([eng, ref], acts)
            after = eng.inc_stats()
            assert (after[0] - before[0], after[1] - before[1]) == (want.count("inc"), want.count("full")), (s, before, after, want)
        for sim, a in zip(sims, acts):
            sim.simulate(a)
        if not (short or s in S.LONG_CHECKS):
            continue
        assert eng.status() == 0 and ref.status() == 0
        for i, sim in enumerate(sims):
            name = "%s/%s step %d ring %d" % (wname, sname, s, world.rings[i][0])
            compare_state(eng, i, sim, "incremental, " + name, check_vm=short)
            compare_state(ref, i, sim, "full solve, " + name, check_vm=short)
            _compare_engines(eng, ref, i, name)
            if not short:  # (the virtual map at 1e-6 in the long scripts)
                prob, vinfo, tr, upd = eng.virtual_map(i)
                oprob, ovinfo, otr, oupd = sim.virtual_map()
                np.testing.assert_array_equal(upd, oupd)
                np.testing.assert_allclose(prob, oprob, rtol=1e-14, err_msg=name)
                np.testing.assert_allclose(vinfo, ovinfo, rtol=1e-6, atol=1e-9, err_msg=name)
                np.testing.assert_allclose(tr, otr, rtol=1e-6, err_msg=name)
    # both sides of each fallback edge were asserted in this run
    if wname == "large":
        assert {(False, False, "inc"), (True, False, "full")} <= seen_paths
    else:
        assert {(False, False, "inc"), (False, True, "full")} <= seen_paths
    eng.close()
    ref.close()


# --------------------------------------------------------------------------------------- 4. look-ahead from the ring beliefs
_PLANS = [[(0.05, 0.0, 0.01), (-0.05, 0.0, -0.01)], [(-0.04, 0.02, 0.01), (0.05, 0.0, 0.0), (0.03, -0.02, -0.01)]]


def _lookahead_case(world, script, envs, monkeypatch):
    sims = world.make_sims()
    eng = _engine(world, n_roll=2 * len(envs))
    monkeypatch.setenv("DRLGX_LOOKAHEAD_LOOP", "0")
    per_action = _engine(world, n_roll=2 * len(envs))
    monkeypatch.delenv("DRLGX_LOOKAHEAD_LOOP")
    for s, kind in enumerate(script):
        acts = world.actions(sims, kind, s)
        _step([eng, per_action], acts)
        for sim, a in zip(sims, acts):
            sim.simulate(a)
    A = eng.cfg.max_actions
    cand = [(e, p) for e in envs for p in _PLANS]
    acts = np.zeros((len(cand), A, 3))
    for c, (_, p) in enumerate(cand):
        acts[c, :len(p)] = p
    rewards = []
    for g in (eng, per_action):
        ce = torch.tensor([e for e, _ in cand], dtype=torch.int32, device=g.device)
        rewards.append(g.lookahead(ce, torch.tensor(acts, device=g.device), torch.tensor([len(p) for _, p in cand], dtype=torch.int32, device=g.device),
                                   max_n_actions=3).cpu().numpy())
        assert g.status() == 0
    for c, (e, p) in enumerate(cand):
        want = sims[e].simulations_reward(np.array(p))
        print("%s ring %d, %d actions: reward %.9f, oracle %.9f" % (world.name, world.rings[e][0], len(p), rewards[0][c], want))
        assert rewards[0][c] == pytest.approx(want, abs=1e-6), (world.name, e, len(p))
    _assert_bits((rewards[0],), (rewards[1],), "one launch per plan vs one launch per action")
    for i, sim in enumerate(sims):
        compare_state(eng, i, sim, "%s env %d after the look-ahead" % (world.name, i))
    eng.close()
    per_action.close()


@pytest.mark.parametrize("case", ["small33", "large65", "loop129", "loop130"])
def test_lookahead_from_the_ring_beliefs(case, monkeypatch):
    """Two- and three-action plans that stay in the ring, from the short-script beliefs of the rings of 33, 65, 129 and 130: the
    rewards against OracleSim.simulations_reward at 1e-6, one launch per plan bit-equal to one launch per action
    (DRLGX_LOOKAHEAD_LOOP=0), the live state untouched."""
    sim_w = {w.name: w for w in S.sim_worlds()}
    world, script, envs = {"small33": (S.small_world(), S.SHORT, [7]), "large65": (S.large_world(), S.SHORT, [4]),
                           "loop129": (sim_w["loop129"], S.SIM_SCRIPT, [0]), "loop130": (sim_w["loop130"], S.SIM_SCRIPT, [0])}[case]
    assert world.rings[envs[0]][0] == int(case[-3:] if case.startswith("loop") else case[-2:])
    _lookahead_case(world, script, envs, monkeypatch)


# ------------------------------------------------------------------------------------------------------ 5. capacity is a status
@pytest.mark.parametrize("case,caps,script,solo_last", [("factors", dict(max_factors=100), "j", False),
                                                         ("landmarks", dict(max_landmarks=70), "jg", False),
                                                         ("poses", dict(max_poses=4), "jjjj", True)])
def test_capacity_is_a_status(case, caps, script, solo_last):
    """Ring 65 (with a 12-gate) beside ring 8 (the module's docstring says why every store stays inside the instance's slices):
    (factors) max_factors = 100: the reset appends 65, the next measurement would make 130 -> DRLGX_E_CAPACITY; (landmarks)
    max_landmarks = 70: the gate step's 12 first sightings would make 77; (poses) max_poses = 4: the fourth move, and the pose count
    stays 4.  Counts stay within the capacities, the ring-8 instance stays bit-equal to the same instance of an engine with ample
    capacities, and a reset of the overflowed environment clears the status and matches the oracle again."""
    world = S.capacity_world()
    sims = world.make_sims()
    eng, ample = _engine(world, **caps), _engine(world)
    for s, kind in enumerate(script):
        last = s == len(script) - 1
        acts = world.actions(sims, kind, s)
        _step([eng, ample], acts, only=0 if (solo_last and last) else None)
        for e, (sim, a) in enumerate(zip(sims, acts)):
            if not (solo_last and last and e != 0):
                sim.simulate(a)
        assert ample.status() == 0
        assert eng.status() == (DRLGX_E_CAPACITY if last else 0), "%s: step %d" % (case, s)
        c = eng.counts(0)
        assert c["poses"] <= eng.cfg.max_poses and c["landmarks"] <= eng.cfg.max_landmarks and c["factors"] <= eng.cfg.max_factors
        _assert_bits(_dump(eng, 1), _dump(ample, 1), "%s: ring 8 beside the overflow, step %d" % (case, s))
        compare_state(eng, 1, sims[1], "%s: ring 8, step %d" % (case, s))
        assert eng.counts(1) == ample.counts(1)
    if case == "poses":
        assert eng.counts(0)["poses"] == 4 and ample.counts(0)["poses"] == 5
    fresh = world.make_sims()[0]
    eng.reset([0], [0], starts=world.starts[0:1])
    assert eng.status() == 0
    compare_state(eng, 0, fresh, "%s: after the reset of the overflowed environment" % case, check_vm=False)
    acts = world.actions([fresh, sims[1]], "j", 0)
    if case != "factors":  # (with 100 factors the first step overflows again)
        _step([eng], acts, only=0)
        fresh.simulate(acts[0])
        assert eng.status() == 0
        compare_state(eng, 0, fresh, "%s: a step after that reset" % case)
    eng.close()
    ample.close()
