"""GPU tests (run with -m gpu on an MI355X) of the expected map entropy of candidate plans - drlgx_og_cost,
calculateUncertainty_OG_SHANNON and costFunction (csrc/k_og.hip) - against tests/og_ref.py on the maps, beliefs and plans of
tests/og_cases.py (whose margins tests/test_og_cpu.py checks on the CPU).

Tolerances: every cell's probability is compared and must be og_ref's bits - the values are entries of the ladder's table.
Entropy and cost rel 1e-12: at most 400 terms, each <= ln 2 and within a few ulp of the restatement's (the device's log against
the C library's), summed in another order - about 7e-14 relative, a margin of ~14.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import og_cases  # noqa: E402
import og_ref  # noqa: E402

SUM_RTOL = 1e-12
DRLGX_E_INVALID = -1
A = og_cases.MAX_ACTIONS


class Ctx(object):
    """The 3 environments of one map of og_cases stepped through its script beside their oracles (P = 7), and the reference of
    every (environment, plan) computed once.  `cases`: another module or object with og_cases' names (tests/rect_cases.py: OgView)."""

    def __init__(self, name, cases=og_cases):
        from drl_graph_exploration_amd.engine import Engine
        assert cases.MAX_ACTIONS == A
        self.K = cases
        n = cases.N_ENVS
        self.name = name
        self.cfg = cases.engine_config(name)
        self.eng = Engine(self.cfg, n)
        self.sims = cases.make_sims(name)
        self.eng.reset(np.arange(n), np.arange(n), starts=cases.STARTS)
        for act in cases.SCRIPT:
            self.eng.step(torch.tensor([act] * n, dtype=torch.float64, device=self.eng.device))
        assert self.eng.status() == 0
        for e, s in enumerate(self.sims):  # the belief is the oracle's (what the restatement starts from)
            assert self.eng.counts(e)["poses"] == s.num_poses() and self.eng.counts(e)["landmarks"] == s.num_landmarks()
            np.testing.assert_allclose(self.eng.poses(e)[0], s.poses()[0], atol=1e-9)
            np.testing.assert_allclose(self.eng.landmarks(e)[1], s.landmarks()[1], atol=1e-9)
        self.plans = [cases.plans_for(s) for s in self.sims]
        self.cases = [(e, k) for e in range(n) for k in range(len(self.plans[e]))]
        self._ref = {}

    def ref(self, e, k):
        if (e, k) not in self._ref:
            self._ref[(e, k)] = og_ref.og_cost(self.sims[e], self.plans[e][k])[:3]
        return self._ref[(e, k)]

    def device_candidates(self, cases):
        acts = np.zeros((len(cases), A, 3))
        for c, (e, k) in enumerate(cases):
            acts[c, :len(self.plans[e][k])] = np.reshape(self.plans[e][k], (-1, 3))
        dev = self.eng.device
        return (torch.tensor([e for e, _ in cases], dtype=torch.int32, device=dev), torch.tensor(acts, device=dev),
                torch.tensor([len(self.plans[e][k]) for e, k in cases], dtype=torch.int32, device=dev))

    def live_state(self):
        out = []
        for e in range(self.K.N_ENVS):
            out += list(self.eng.poses(e)) + list(self.eng.landmarks(e)) + list(self.eng.virtual_map(e))
        return out

    def check(self, case, ent, cost, prob, tag):
        rh, rc, rp = self.ref(*case)
        print("%s: prob cells differing %d  entropy %.2e  cost %.2e" % (tag, int(np.sum(prob != rp)), abs(ent / rh - 1), abs(cost / rc - 1)))
        np.testing.assert_array_equal(prob, rp, err_msg=tag)  # every cell
        assert ent == pytest.approx(rh, rel=SUM_RTOL), tag
        assert cost == pytest.approx(rc, rel=SUM_RTOL), tag


_ctx = {}


@pytest.fixture(scope="module")
def ctx():
    def get(name):
        if name not in _ctx:
            _ctx[name] = Ctx(name)
        return _ctx[name]
    yield get
    for c in _ctx.values():
        c.eng.close()
    _ctx.clear()


def _assert_same(before, after):
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", sorted(og_cases.CONFIGS))
def test_parity_with_the_restatement(ctx, name):
    """36 cells (less than a wave, a partial tile), 400 cells (20 is no multiple of 8) and the narrow sensor (the bounding box
    prunes): K = 0, 1, max_actions, P + K = 63, 64, 65, a plan that leaves the map box; landmark estimates outside the grid;
    candidates that share an environment.  The live state is read only."""
    c = ctx(name)
    assert (c.eng.rows * c.eng.cols) == {"small": 36, "mid": 400, "sector": 36}[name]
    if name == "small":
        assert sum(og_cases.landmarks_outside_the_grid(s) for s in c.sims) > 0
    assert all(og_cases.leaves_the_map(c.sims[e], c.plans[e][6]) for e in range(og_cases.N_ENVS))
    before = c.live_state()
    ce, acts, nact = c.device_candidates(c.cases)
    ent, cost, prob = c.eng.og_cost(ce, acts, nact, want_prob=True)
    assert c.eng.status() == 0
    ent, cost, prob = ent.cpu().numpy(), cost.cpu().numpy(), prob.cpu().numpy()
    for i, case in enumerate(c.cases):
        c.check(case, ent[i], cost[i], prob[i], "%s env %d plan %d" % ((name,) + case))
    _assert_same(before, c.live_state())


def test_pose_counts_around_64_with_variants_picked_by_capacity(monkeypatch):
    """P + K = 63, 64, 65 again on an engine that picks its kernel variants by max_poses (as if every trajectory were full)."""
    monkeypatch.setenv("DRLGX_VARIANT_BY_CAPACITY", "1")
    c = Ctx("small")
    try:
        cases = [(e, k) for e, k in c.cases if k in (3, 4, 5)]
        ce, acts, nact = c.device_candidates(cases)
        assert sorted(set((nact + 7).tolist())) == [63, 64, 65]
        ent, cost, prob = (t.cpu().numpy() for t in c.eng.og_cost(ce, acts, nact, want_prob=True))
        assert c.eng.status() == 0
        for i, case in enumerate(cases):
            c.check(case, ent[i], cost[i], prob[i], "by capacity env %d plan %d" % case)
    finally:
        c.eng.close()


def test_zero_actions_give_the_live_map(ctx):
    for name in sorted(og_cases.CONFIGS):
        c = ctx(name)
        n = og_cases.N_ENVS
        dev = c.eng.device
        ent, cost, prob = c.eng.og_cost(torch.arange(n, dtype=torch.int32, device=dev), torch.zeros(n, A, 3, dtype=torch.float64, device=dev),
                                        torch.zeros(n, dtype=torch.int32, device=dev), want_prob=True)
        assert torch.equal(ent, cost)  # no action, no distance
        for e in range(n):
            np.testing.assert_array_equal(prob[e].cpu().numpy(), c.eng.virtual_map(e)[0])
        assert c.eng.status() == 0


def test_candidate_counts_duplicates_and_determinism(ctx):
    """n_cand = 0, 1 and 257 (more workgroups than compute units), cycling the parity cases: a repeated (environment, plan) pair
    gets the same bits, a second call gets the same bits, and the last candidate matches the restatement."""
    c = ctx("mid")
    dev = c.eng.device
    empty = c.eng.og_cost(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, A, 3, dtype=torch.float64, device=dev),
                          torch.zeros(0, dtype=torch.int32, device=dev), want_prob=True)
    assert [t.numel() for t in empty] == [0, 0, 0]
    one = c.device_candidates(c.cases[2:3])
    ent, cost, prob = (t.cpu().numpy() for t in c.eng.og_cost(*one, want_prob=True))
    c.check(c.cases[2], ent[0], cost[0], prob[0], "one candidate")
    cases = [c.cases[i % len(c.cases)] for i in range(257)]
    ce, acts, nact = c.device_candidates(cases)
    out = [c.eng.og_cost(ce, acts, nact, want_prob=True), c.eng.og_cost(ce, acts, nact, want_prob=True)]
    assert c.eng.status() == 0
    (ent, cost, prob), again = [[t.cpu().numpy() for t in o] for o in out]
    _assert_same((ent, cost, prob), again)
    first = {}
    for i, case in enumerate(cases):
        f = first.setdefault(case, i)
        assert ent[i] == ent[f] and cost[i] == cost[f], i
        np.testing.assert_array_equal(prob[i], prob[f])
    assert len(first) == len(c.cases)
    c.check(cases[256], ent[256], cost[256], prob[256], "candidate 256")
    # entropy only / cost only give the same bits as both
    e_only = torch.empty(257, dtype=torch.float64, device=dev)
    c_only = torch.empty(257, dtype=torch.float64, device=dev)
    assert _raw_og_cost(c.eng, ce, acts, nact, e_only, None) == 0 and _raw_og_cost(c.eng, ce, acts, nact, None, c_only) == 0
    np.testing.assert_array_equal(e_only.cpu().numpy(), ent)
    np.testing.assert_array_equal(c_only.cpu().numpy(), cost)


def _raw_og_cost(eng, ce, acts, nact, ent, cost, prob=None):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return eng.L.drlgx_og_cost(eng.h, ce.numel(), p(ce), p(acts), p(nact), p(ent), p(cost), p(prob))


def test_bad_arguments_are_refused_before_anything_runs(ctx):
    c = ctx("small")
    eng = c.eng
    before = c.live_state()
    ce, acts, nact = c.device_candidates(c.cases[:3])
    ent = torch.full((3,), -7.0, dtype=torch.float64, device=eng.device)
    cost = torch.full((3,), -7.0, dtype=torch.float64, device=eng.device)
    prob = torch.full((3, eng.rows, eng.cols), -7.0, dtype=torch.float64, device=eng.device)
    assert _raw_og_cost(eng, ce, acts, nact, None, None, prob) == DRLGX_E_INVALID       # both scalar outputs NULL
    too_long = nact.clone()
    too_long[1] = A + 1
    assert _raw_og_cost(eng, ce, acts, too_long, ent, cost, prob) == DRLGX_E_INVALID    # n_actions beyond max_actions
    nowhere = ce.clone()
    nowhere[2] = og_cases.N_ENVS
    assert _raw_og_cost(eng, nowhere, acts, nact, ent, cost, prob) == DRLGX_E_INVALID   # a candidate that names no environment
    assert eng.status() == 0
    assert float(ent.min()) == -7.0 and float(cost.max()) == -7.0 and float(prob.max()) == -7.0  # nothing was written
    _assert_same(before, c.live_state())
    # the expected EM cost still has no third algorithm
    assert eng.L.drlgx_em_cost(eng.h, 3, C.c_void_p(ce.data_ptr()), C.c_void_p(acts.data_ptr()), C.c_void_p(nact.data_ptr()), 2,
                               C.c_void_p(ent.data_ptr()), C.c_void_p(cost.data_ptr()), None) == DRLGX_E_INVALID
    assert eng.status() == 0 and float(ent.min()) == -7.0
    assert _raw_og_cost(eng, ce, acts, nact, ent, cost, prob) == 0
    assert float(ent.min()) > 0 and float(cost.min()) > 0 and float(prob.min()) > 0


def test_planner_facade_leaf_entropy():
    from staged_facade import StagedEMExplorer
    from test_gpu_modules import ini
    from oracle import oracle as O
    lo = 6
    start = tuple(np.array(O.start_pose(lo, 40 / 2 + 20)) + np.array([0.3113, 0.2291, -0.0517]))
    ex = StagedEMExplorer(ini(lo), start=start, max_poses=16)
    for _ in range(4):
        ex.simulate((1, 1, math.pi / 2.0))
    eng = ex.engine
    plan = [(0.0, 0.0, 0.6), (2.0, 0.0, 0.0), (1.2, 0.0, 0.0)]
    acts = torch.zeros(1, eng.cfg.max_actions, 3, dtype=torch.float64, device=eng.device)
    acts[0, :3] = torch.tensor(plan, dtype=torch.float64)
    ent, cost = eng.og_cost(torch.zeros(1, dtype=torch.int32, device=eng.device), acts, torch.tensor([3], dtype=torch.int32, device=eng.device))
    h, hc = ex._planner.leaf_entropy(ex._slam, ex._virtual_map, plan, return_cost=True)
    assert (h, hc) == (float(ent[0]), float(cost[0])) and hc > h > 0
    assert ex._planner.leaf_entropy(ex._slam, ex._virtual_map, plan) == h
    eng.check_status()


def test_vec_env_rewards_from_the_expected_entropy():
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    import em_cases
    n = 4
    env = VecExplorationEnv(em_cases.MAP, n, env_index=0, test=True, starts=em_cases.generic_starts(n), max_poses=60, n_rollouts=7)
    g = env.graph_matrix()
    actions, n_act = env.actions_all_goals()
    r, raw = env.rewards_all_goals(lookahead="og", return_raw=True)
    cand_env, _, first = env.candidates
    dev = env.engine.device
    _, cost = env.engine.og_cost(cand_env, actions, n_act)
    root, _ = env.engine.og_cost(torch.arange(n, dtype=torch.int32, device=dev), torch.zeros(n, actions.shape[1], 3, dtype=torch.float64, device=dev),
                                 torch.zeros(n, dtype=torch.int32, device=dev))
    assert torch.equal(raw, root[cand_env.long()] - cost)
    r_h, raw_h, first_h, nfr = r.cpu().numpy(), raw.cpu().numpy(), first.cpu().numpy(), g["n_frontier_h"]
    assert np.all(r_h >= -1.0) and np.all(r_h <= 1.0)
    for e in range(n):  # exploration_env.py:151-161: the arg-max goes to 0 when it is the nearest frontier, else to 1
        seg = slice(first_h[e], first_h[e] + nfr[e])
        if nfr[e] > 1 and raw_h[seg].max() > raw_h[seg].min():
            best = int(np.argmax(raw_h[seg]))
            assert r_h[seg][best] == (0.0 if best == 0 else 1.0) and r_h[seg].min() == -1.0
    with pytest.raises(ValueError):
        env.rewards_all_goals(lookahead="shannon")
    env.engine.check_status()
    env.close()
