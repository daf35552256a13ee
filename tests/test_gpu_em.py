"""GPU tests (run with -m gpu on an MI355X) of the expected look-ahead cost of candidate plans - drlgx_em_cost, the leaf
evaluation of EMPlanner2D::optimize2 (csrc/k_em.hip) - against tests/em_ref.py on the beliefs and plans of tests/em_cases.py
(whose margins tests/test_em_cpu.py checks on the CPU).

Tolerances: the cells' information and the A-opt values rel 1e-6 - the project's tolerance for the fm2 covariances that feed
them (the map algebra itself is held at 1e-7); the D-opt values rel 8.9e-9 = 10 x the largest move of
em_ref's own D-opt value under 1e-6 relative perturbations of its input covariances (8.84e-10, measured on the CPU over all
parity cases).  Which cells stay at I / sigma0^2 must agree exactly.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_cases  # noqa: E402
import em_ref  # noqa: E402
from oracle import fm2_ref  # noqa: E402
from test_gpu_belief import compare_state, make_engine  # noqa: E402

INFO_RTOL = AOPT_RTOL = 1e-6
DOPT_RTOL = 8.9e-9
DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3


class Ctx(object):
    """4 environments stepped through the first 11 actions of the shared script beside their oracles (P = 12), the parity
    candidates on the device, and the reference of every (environment, plan) computed once."""

    def __init__(self):
        n = em_cases.N_ENVS
        self.eng, self.cfg = make_engine(n, num_landmarks=em_cases.NUM_LANDMARKS, max_poses=64)
        self.sims, starts = em_cases.make_sims(n)
        self.eng.reset(np.arange(n), np.arange(n), starts=starts)
        for act in em_cases.SCRIPT:
            self.eng.step(torch.tensor([act] * n, dtype=torch.float64, device=self.eng.device))
        assert self.eng.status() == 0
        self.A = self.cfg.max_actions
        self.plans = [em_cases.plans_for(s, self.A) for s in self.sims]
        self.cases = [(e, k) for e in range(n) for k in range(len(self.plans[e]))]
        self._ref = {}

    def ref(self, e, k):
        if (e, k) not in self._ref:
            self._ref[(e, k)] = em_ref.em_costs(self.sims[e], self.plans[e][k])
        return self._ref[(e, k)]

    def device_candidates(self, cases):
        acts = np.zeros((len(cases), self.A, 3))
        for c, (e, k) in enumerate(cases):
            acts[c, :len(self.plans[e][k])] = np.reshape(self.plans[e][k], (-1, 3))
        dev = self.eng.device
        return (torch.tensor([e for e, _ in cases], dtype=torch.int32, device=dev), torch.tensor(acts, device=dev),
                torch.tensor([len(self.plans[e][k]) for e, k in cases], dtype=torch.int32, device=dev))


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.eng.close()


def _untouched(info, sigma0):
    i0 = 1.0 / sigma0 ** 2
    return (info[..., 0] == i0) & (info[..., 1] == 0.0) & (info[..., 2] == i0)


def _check_against_ref(ctx, e, k, unc0, cost0, unc1, cost1, info, tag):
    (ru0, rc0), (ru1, rc1), rinfo, _ = ctx.ref(e, k)
    info = info.reshape(-1, 3)
    gap = np.abs(info - rinfo) / np.maximum(np.abs(rinfo), 1e-9)
    print("%s: info %.2e  aopt %.2e cost %.2e  dopt %.2e cost %.2e" % (tag, gap.max(), abs(unc0 / ru0 - 1), abs(cost0 / rc0 - 1),
                                                                      abs(unc1 / ru1 - 1), abs(cost1 / rc1 - 1)))
    np.testing.assert_array_equal(_untouched(info, ctx.sims[e].cfg.sigma0), _untouched(rinfo, ctx.sims[e].cfg.sigma0), err_msg=tag)
    np.testing.assert_allclose(info, rinfo, rtol=INFO_RTOL, atol=1e-9, err_msg=tag)
    assert unc0 == pytest.approx(ru0, rel=AOPT_RTOL), tag
    assert cost0 == pytest.approx(rc0, rel=AOPT_RTOL), tag
    assert unc1 == pytest.approx(ru1, rel=DOPT_RTOL), tag
    assert cost1 == pytest.approx(rc1, rel=DOPT_RTOL), tag


@pytest.mark.parametrize("env", range(em_cases.N_ENVS))
def test_parity_with_the_restatement(ctx, env):
    """The three fm2 plans, no action, a pure rotation, a max_actions-long plan and a jump away from every estimated landmark:
    info, uncertainty (both algorithms) and cost against em_ref; no case on a knife edge (nothing is skipped)."""
    cases = [(e, k) for e, k in ctx.cases if e == env]
    ce, acts, nact = ctx.device_candidates(cases)
    unc0, cost0, info = ctx.eng.em_cost(ce, acts, nact, 0, want_info=True)
    unc1, cost1 = ctx.eng.em_cost(ce, acts, nact, 1)
    assert ctx.eng.status() == 0
    unc0, cost0, info, unc1, cost1 = (t.cpu().numpy() for t in (unc0, cost0, info, unc1, cost1))
    n_meas = [sum(fm2_ref.fm2_update(ctx.sims[e], ctx.plans[e][k])[1]) for e, k in cases]
    assert len(ctx.plans[env][5]) == ctx.A and n_meas[6] == 0 and n_meas[3] == 0 and max(n_meas) > 3
    for c, (e, k) in enumerate(cases):
        assert min(ctx.ref(e, k)[3].values()) > 1e-9, "case (%d, %d) sits on a knife edge: choose another plan" % (e, k)
        _check_against_ref(ctx, e, k, unc0[c], cost0[c], unc1[c], cost1[c], info[c], "env %d plan %d" % (e, k))


def test_zero_actions_equal_the_live_map(ctx):
    n = em_cases.N_ENVS
    dev = ctx.eng.device
    ce = torch.arange(n, dtype=torch.int32, device=dev)
    acts = torch.zeros(n, ctx.A, 3, dtype=torch.float64, device=dev)
    nact = torch.zeros(n, dtype=torch.int32, device=dev)
    for alg in (0, 1):
        unc, cost, info = ctx.eng.em_cost(ce, acts, nact, alg, want_info=True)
        live = ctx.eng.uncertainty_em(alg).cpu().numpy()
        unc, cost, info = unc.cpu().numpy(), cost.cpu().numpy(), info.cpu().numpy()
        for e in range(n):
            vinfo = ctx.eng.virtual_map(e)[1]
            want = np.stack([vinfo[:, 0, 0], vinfo[:, 0, 1], vinfo[:, 1, 1]], axis=1)
            got = info[e].reshape(-1, 3)
            print("alg %d env %d: unc %.2e info %.2e" % (alg, e, abs(unc[e] / live[e] - 1), (np.abs(got - want) / np.maximum(np.abs(want), 1e-9)).max()))
            assert unc[e] == pytest.approx(live[e], rel=1e-7)
            assert cost[e] == unc[e]
            np.testing.assert_array_equal(_untouched(got, ctx.cfg.sigma0), ctx.eng.virtual_map(e)[3] == 0)
            np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-9)
    assert ctx.eng.status() == 0


def test_chunks_and_duplicates(ctx):
    """130 candidates (more than one chunk of 128) cycling the parity cases: a repeated (environment, plan) pair gets the same
    bits, a second call gets the same bits, and the candidate behind the chunk boundary matches the restatement."""
    cases = [ctx.cases[c % len(ctx.cases)] for c in range(130)]
    ce, acts, nact = ctx.device_candidates(cases)
    out = [ctx.eng.em_cost(ce, acts, nact, 0, want_info=True), ctx.eng.em_cost(ce, acts, nact, 0, want_info=True)]
    unc1, cost1 = ctx.eng.em_cost(ce, acts, nact, 1)
    assert ctx.eng.status() == 0
    (unc, cost, info), again = [[t.cpu().numpy() for t in o] for o in out]
    for a, b in zip((unc, cost, info), again):
        np.testing.assert_array_equal(a, b)
    first = {}
    for c, case in enumerate(cases):
        f = first.setdefault(case, c)
        assert unc[c] == unc[f] and cost[c] == cost[f], c
        np.testing.assert_array_equal(info[c], info[f])
    assert len(first) == len(ctx.cases) and 129 not in first.values()
    e, k = cases[129]
    _check_against_ref(ctx, e, k, unc[129], cost[129], float(unc1[129]), float(cost1[129]), info[129], "candidate 129")


def test_fm2_update_is_unchanged_by_em_cost(ctx):
    ce, acts, nact = ctx.device_candidates(ctx.cases)
    cov0, n0 = ctx.eng.fm2_update(ce, acts, nact)
    ctx.eng.em_cost(ce, acts, nact, 1, want_info=True)
    cov1, n1 = ctx.eng.fm2_update(ce, acts, nact)
    assert ctx.eng.status() == 0
    n0, n1, cov0, cov1 = n0.cpu().numpy(), n1.cpu().numpy(), cov0.cpu().numpy(), cov1.cpu().numpy()
    np.testing.assert_array_equal(n0, n1)
    for c in range(len(ctx.cases)):
        np.testing.assert_array_equal(cov0[c, :n0[c]], cov1[c, :n1[c]])
    # ... and they still are the restatement's (what test_fm2_covariance_update_matches_the_restatement checks)
    e, k = ctx.cases[2]
    np.testing.assert_allclose(cov1[2, :n1[2]], fm2_ref.fm2_update(ctx.sims[e], ctx.plans[e][k])[0], rtol=1e-6, atol=1e-10)


def _raw_em_cost(eng, ce, acts, nact, alg, unc, cost):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return eng.L.drlgx_em_cost(eng.h, ce.numel(), p(ce), p(acts), p(nact), alg, p(unc), p(cost), None)


def test_bad_arguments_are_refused_before_anything_runs(ctx):
    eng = ctx.eng
    ce, acts, nact = ctx.device_candidates(ctx.cases[:3])
    unc = torch.full((3,), -7.0, dtype=torch.float64, device=eng.device)
    cost = torch.full((3,), -7.0, dtype=torch.float64, device=eng.device)
    assert _raw_em_cost(eng, ce, acts, nact, 2, unc, cost) == DRLGX_E_INVALID          # a bad algorithm
    assert _raw_em_cost(eng, ce, acts, nact, 0, None, None) == DRLGX_E_INVALID         # both outputs NULL
    too_long = nact.clone()
    too_long[1] = ctx.A + 1
    assert _raw_em_cost(eng, ce, acts, too_long, 0, unc, cost) == DRLGX_E_INVALID      # n_actions beyond max_actions
    nowhere = ce.clone()
    nowhere[2] = em_cases.N_ENVS
    assert _raw_em_cost(eng, nowhere, acts, nact, 0, unc, cost) == DRLGX_E_INVALID     # a candidate that names no environment
    assert eng.status() == 0
    assert float(unc.min()) == -7.0 and float(cost.max()) == -7.0                      # nothing was written
    assert _raw_em_cost(eng, ce, acts, nact, 0, unc, None) == 0 and _raw_em_cost(eng, ce, acts, nact, 0, None, cost) == 0
    assert float(unc.min()) > 0 and float(cost.min()) > 0
    for i in range(em_cases.N_ENVS):
        compare_state(eng, i, ctx.sims[i], "after refused calls env %d" % i)


def test_more_than_256_predicted_measurements_are_refused():
    """40 listed landmarks on a ring of 3 m around the start: the reset sights them all, so 8 short actions predict 320
    measurements - DRLGX_E_CAPACITY from the argument check, the status word stays 0."""
    import math
    n_lm = 40
    eng, cfg = make_engine(1, num_landmarks=n_lm, max_poses=64)
    start = np.array([[1.3183, -2.2718, 0.6234]])
    ang = start[0, 2] + (np.arange(n_lm) + 0.5) * 2 * math.pi / n_lm
    eng.set_fixed_landmarks(np.stack([start[0, 0] + 3.0 * np.cos(ang), start[0, 1] + 3.0 * np.sin(ang)], axis=1))
    eng.reset(np.array([0]), np.array([0]), starts=start)
    assert eng.status() == 0 and eng.counts(0)["landmarks"] == n_lm
    dev = eng.device
    ce = torch.zeros(1, dtype=torch.int32, device=dev)
    acts = torch.zeros(1, cfg.max_actions, 3, dtype=torch.float64, device=dev)
    acts[0, :8] = torch.tensor([0.05, 0.0, 0.01], dtype=torch.float64)
    unc = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    assert _raw_em_cost(eng, ce, acts, torch.tensor([8], dtype=torch.int32, device=dev), 0, unc, None) == DRLGX_E_CAPACITY
    assert eng.status() == 0 and float(unc[0]) == -7.0
    assert _raw_em_cost(eng, ce, acts, torch.tensor([6], dtype=torch.int32, device=dev), 0, unc, None) == 0  # 240 measurements
    assert eng.status() == 0 and float(unc[0]) > 0
    eng.close()


def test_vec_env_rewards_from_the_expected_cost():
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    n = 4
    env = VecExplorationEnv(em_cases.MAP, n, env_index=0, test=True, starts=em_cases.generic_starts(n), max_poses=60, n_rollouts=7)
    g = env.graph_matrix()
    actions, n_act = env.actions_all_goals()
    r, raw = env.rewards_all_goals(lookahead="em", return_raw=True)
    cand_env, _, first = env.candidates
    alg = int(env.cfg.algorithm)
    _, cost = env.engine.em_cost(cand_env, actions, n_act, alg)
    want = env.engine.uncertainty_em(alg)[cand_env.long()] - cost
    assert torch.equal(raw, want)
    r_h, raw_h, first_h, nfr = r.cpu().numpy(), raw.cpu().numpy(), first.cpu().numpy(), g["n_frontier_h"]
    assert np.all(r_h >= -1.0) and np.all(r_h <= 1.0)
    for e in range(n):  # exploration_env.py:151-161: the arg-max goes to 0 when it is the nearest frontier, else to 1
        seg = slice(first_h[e], first_h[e] + nfr[e])
        if nfr[e] > 1 and raw_h[seg].max() > raw_h[seg].min():
            best = int(np.argmax(raw_h[seg]))
            assert r_h[seg][best] == (0.0 if best == 0 else 1.0) and r_h[seg].min() == -1.0
            assert bool(env.loop_clo[e]) == (best != 0)
    sim_default, raw_default = env.rewards_all_goals(return_raw=True)
    sim_named, raw_named = env.rewards_all_goals(return_raw=True, lookahead="sim")
    assert torch.equal(sim_default, sim_named) and torch.equal(raw_default, raw_named)
    with pytest.raises(ValueError):
        env.rewards_all_goals(lookahead="both")
    env.engine.check_status()
    env.close()


def test_live_state_is_untouched(ctx):
    """Last of the tests on the shared engine: after every em_cost call above (and one more here) the environments still are
    their oracles', and the next belief step matches the oracle's."""
    ce, acts, nact = ctx.device_candidates(ctx.cases)
    ctx.eng.em_cost(ce, acts, nact, 0, want_info=True)
    n = em_cases.N_ENVS
    for i in range(n):
        compare_state(ctx.eng, i, ctx.sims[i], "after em_cost env %d" % i)
    act = (1.3, 0.0, 0.4)
    ctx.eng.step(torch.tensor([act] * n, dtype=torch.float64, device=ctx.eng.device))
    for s in ctx.sims:
        s.simulate(act)
    assert ctx.eng.status() == 0
    for i in range(n):
        compare_state(ctx.eng, i, ctx.sims[i], "step after em_cost env %d" % i)
    ctx._ref.clear()  # (the belief moved on)
