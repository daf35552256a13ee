"""GPU tests (run with -m gpu on an MI355X) of optimize2's tree under OG_SHANNON / SLAM_OG_SHANNON - drlgx_og_plan: the tree of
drlgx_em_plan, the leaf costs of drlgx_og_cost / drlgx_slam_og_cost computed from a base that the leaves of a tree share
(csrc/k_og.hip: k_og_tree_base, k_og_tree_cost) - on the world of tests/og_plan_cases.py: a 13 x 21 map (partial last tiles), P = 1
without a landmark, P = 10 and P = 67, two landmarks in one cell.

What is compared how:
  * the tree against drlgx_em_plan's from the same Halton starts: equal arrays;
  * every leaf's cost against Engine.og_cost / Engine.slam_og_cost on the leaves that em_plan_leaves() reports: the same BITS, with
    the shared base (the default) and with DRLGX_OG_TREE_SHARED=0 (an engine created under the switch), and the two engines against
    each other;
  * the leaves' entropies against tests/og_ref.py at tests/test_gpu_og.py's SUM_RTOL, algorithm 3's uncertainties against
    tests/slam_og_ref.py through tests/slam_og_check.py's check_case (tests/test_gpu_slam_og.py's tolerances), on the oracles'
    beliefs - whose decision margins are asserted here (1e-6 m: the engine's belief follows the oracle's to 1e-9);
  * the pick against a host arg-min with optimize2's rule: equal arrays.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_safe_cases  # noqa: E402
import og_plan_cases as K  # noqa: E402
import og_ref  # noqa: E402
import slam_og_ref  # noqa: E402
from slam_og_check import bits, check_case, live_state  # noqa: E402
from test_gpu_og import SUM_RTOL  # noqa: E402

DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3
SUCCESS = 3
SMALL, MID, BIG = 0.5, 1.5, 5.0   # max_nodes: a dozen leaves for the restatements; ~120 samples; more than 128 leaves (fm2 chunks)
MARGIN = 1e-6


class Ctx(object):
    def __init__(self, max_actions=K.MAX_ACTIONS):
        self.eng, self.cfg = K.make_engine(max_actions)
        self.dev = self.eng.device
        self._sims, self._runs = None, {}

    @property
    def sims(self):
        if self._sims is None:
            self._sims = K.make_sims()
            for e, s in enumerate(self._sims):  # the belief is the oracle's (what the restatements start from)
                assert self.eng.counts(e)["poses"] == s.num_poses() == K.POSES[e]
                assert self.eng.counts(e)["landmarks"] == s.num_landmarks()
                np.testing.assert_allclose(self.eng.poses(e)[0], s.poses()[0], atol=1e-9)
                np.testing.assert_allclose(self.eng.landmarks(e)[1], s.landmarks()[1], atol=1e-9)
        return self._sims

    def i32(self, v):
        return torch.tensor(v, dtype=torch.int32, device=self.dev)

    def state(self):
        return live_state(self.eng, K.N_ENVS) + [self.eng.counts_dev().cpu().numpy()] + \
            [np.asarray(a).copy() for e in range(K.N_ENVS) for a in self.eng.virtual_map(e)]

    def plan(self, alg, max_nodes=SMALL, sel=None, safe_distance=0.0, alpha=K.ALPHA):
        """(outputs, leaves) of one og_plan call on the host, computed once per argument set."""
        sel = list(range(K.N_ENVS)) if sel is None else sel
        key = (alg, max_nodes, tuple(sel), safe_distance, alpha)
        if key not in self._runs:
            self.eng.set_sampler_parameter(max_nodes, safe_distance)
            o = self.eng.og_plan(self.i32(sel), self.i32([K.START_INDICES[e] for e in sel]), K.CAP, alg, alpha, want_nodes=True)
            assert self.eng.status() == 0
            self._runs[key] = (host(o), self.eng.em_plan_leaves())
        return self._runs[key]

    def recost(self, lv, alg, alpha=K.ALPHA):
        """The cost entry on the reported leaves."""
        if alg == 2:
            return self.eng.og_cost(lv["cand_env"], lv["actions"], lv["n_actions"])[1].cpu().numpy()
        return self.eng.slam_og_cost(lv["cand_env"], lv["actions"], lv["n_actions"], alpha)[1].cpu().numpy()


def host(o):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.eng.close()


@pytest.fixture(scope="module")
def unshared():
    """The same world on an engine created under DRLGX_OG_TREE_SHARED=0: k_og_cost on the materialised leaves."""
    mp = pytest.MonkeyPatch()
    mp.setenv("DRLGX_OG_TREE_SHARED", "0")
    try:
        c = Ctx()
    finally:
        mp.undo()
    yield c
    c.eng.close()


def same_bits(a, b, msg=""):
    np.testing.assert_array_equal(bits(np.asarray(a, dtype=np.float64)), bits(np.asarray(b, dtype=np.float64)), err_msg=msg)


def check_same_tree(ctx, max_nodes, safe_distance=0.0):
    o, _ = ctx.plan(2, max_nodes, safe_distance=safe_distance)
    ctx.eng.set_sampler_parameter(max_nodes, safe_distance)
    em = host(ctx.eng.em_plan(ctx.i32(list(range(K.N_ENVS))), ctx.i32(K.START_INDICES), K.CAP, 0, want_nodes=True))
    assert ctx.eng.status() == 0
    for k in ("nodes", "n_nodes", "halton_next", "n_leaves", "result"):
        np.testing.assert_array_equal(o[k], em[k], err_msg=k)
    return o


def check_same_bits_as_the_cost_entry(c, alg, max_nodes, safe_distance=0.0):
    before = c.state()
    o, lv = c.plan(alg, max_nodes, safe_distance=safe_distance)
    assert int(o["n_leaves"].sum()) == lv["cand_env"].numel() and lv["distance"] is None and bool((lv["core"] == 1).all())
    same_bits(lv["cost"].cpu().numpy(), c.recost(lv, alg), "algorithm %d" % alg)
    assert c.eng.status() == 0
    for a, b in zip(before, c.state()):  # live state is only read
        np.testing.assert_array_equal(a, b)
    return o, lv


def test_world_is_what_it_claims(ctx):
    assert (ctx.eng.rows, ctx.eng.cols) == (K.ROWS, K.COLS) and K.ROWS % 8 and K.COLS % 8
    assert [ctx.eng.counts(e)["poses"] for e in range(K.N_ENVS)] == K.POSES and K.POSES[2] > 64
    assert [e for e in range(K.N_ENVS) if ctx.eng.counts(e)["landmarks"] == 0] == K.NO_LANDMARK
    assert ctx.eng.counts(2)["landmarks"] == len(K.LANDMARKS)
    cfg = ctx.cfg
    cells = [(int(math.floor((y - cfg.map_min_y) / cfg.resolution)), int(math.floor((x - cfg.map_min_x) / cfg.resolution)))
             for x, y in ctx.eng.landmarks(2)[1]]
    assert cells.count(K.SHARED_CELL) == 2


def test_same_tree_as_em_plan(ctx):
    o = check_same_tree(ctx, SMALL)
    assert (o["result"] == SUCCESS).all() and o["n_leaves"][0] == 1 and min(o["n_leaves"][1:]) > 3


@pytest.mark.parametrize("alg", [2, 3])
@pytest.mark.parametrize("shared", [True, False])
def test_leaf_costs_are_the_cost_entrys_bits(ctx, unshared, alg, shared):
    c = ctx if shared else unshared
    o, lv = check_same_bits_as_the_cost_entry(c, alg, SMALL)
    if not shared:  # ... and the two paths against each other
        same_bits(lv["cost"].cpu().numpy(), ctx.plan(alg, SMALL)[1]["cost"].cpu().numpy())
        for k, v in ctx.plan(alg, SMALL)[0].items():
            np.testing.assert_array_equal(o[k], v, err_msg=k)
    cost = lv["cost"].cpu().numpy()
    env = lv["cand_env"].cpu().numpy()
    assert len(set(cost[env == 2])) > 1


def test_entropy_against_the_restatement(ctx):
    _, lv = ctx.plan(2, SMALL)
    n = lv["cand_env"].numel()
    assert n <= 40
    ent, cost = (t.cpu().numpy() for t in ctx.eng.og_cost(lv["cand_env"], lv["actions"], lv["n_actions"]))
    same_bits(cost, lv["cost"].cpu().numpy())
    env, acts, nact = lv["cand_env"].cpu().numpy(), lv["actions"].cpu().numpy(), lv["n_actions"].cpu().numpy()
    for i in range(n):
        h, hc, _, margins = og_ref.og_cost(ctx.sims[env[i]], acts[i, :nact[i]])
        print("leaf %d env %d K %d: entropy %.2e cost %.2e margins %s" % (i, env[i], nact[i], abs(ent[i] / h - 1), abs(cost[i] / hc - 1), margins))
        assert min(margins[k] for k in ("range", "bearing", "floor")) > MARGIN
        assert ent[i] == pytest.approx(h, rel=SUM_RTOL) and cost[i] == pytest.approx(hc, rel=SUM_RTOL)


def test_slam_og_uncertainty_against_the_restatement(ctx):
    _, lv = ctx.plan(3, SMALL)
    n = lv["cand_env"].numel()
    assert n <= 40
    out = ctx.eng.slam_og_cost(lv["cand_env"], lv["actions"], lv["n_actions"], K.ALPHA, want_terms=True, want_lm_cov=True)
    out = dict(zip(("unc", "cost", "terms", "weights", "lm_cov"), (t.cpu().numpy() for t in out)))
    same_bits(out["cost"], lv["cost"].cpu().numpy())
    env, acts, nact = lv["cand_env"].cpu().numpy(), lv["actions"].cpu().numpy(), lv["n_actions"].cpu().numpy()
    checked = 0
    for i in range(n):
        if env[i] in K.NO_LANDMARK:  # w1 = inf, NaN - nothing to restate
            assert math.isnan(out["cost"][i])
            continue
        sim, plan = ctx.sims[env[i]], [tuple(a) for a in acts[i, :nact[i]]]
        assert min(og_ref.og_cost(sim, plan)[3][k] for k in ("range", "bearing", "floor")) > MARGIN
        check_case(sim, env[i], "leaf %d" % i, slam_og_ref.slam_og_cost(sim, plan, K.ALPHA), out, i, sum_rtol=SUM_RTOL)
        checked += 1
    assert checked > 6


@pytest.mark.parametrize("alg,max_nodes", [(2, SMALL), (3, SMALL), (3, BIG)])
def test_the_pick(ctx, alg, max_nodes):
    """A host arg-min with optimize2's rule names the leaf.  Under algorithm 3 environment 3 - no landmark, several leaves, every
    cost NaN - must plan to its FIRST leaf: a pick that let a NaN replace the held leaf, or took the last one, fails here."""
    o, lv = ctx.plan(alg, max_nodes)
    cost, acts, nact = lv["cost"].cpu().numpy(), lv["actions"].cpu().numpy(), lv["n_actions"].cpu().numpy()
    off = 0
    for t in range(K.N_ENVS):
        nl = int(o["n_leaves"][t])
        best = off + K.pick(list(cost[off:off + nl]))
        same_bits(o["cost"][t], cost[best])
        assert int(o["n_actions"][t]) == int(nact[best])
        np.testing.assert_array_equal(o["plan"][t], acts[best])
        assert np.all(o["plan"][t, nact[best]:] == 0.0)
        off += nl
    assert off == len(cost)
    if alg == 3:
        env, first = lv["cand_env"].cpu().numpy(), np.concatenate([[0], np.cumsum(o["n_leaves"])])
        assert int(o["n_leaves"][3]) > 1 and int(o["n_leaves"][0]) == 1
        for t in range(K.N_ENVS):
            if t in K.NO_LANDMARK:
                assert np.isnan(cost[env == t]).all() and math.isnan(o["cost"][t])
                np.testing.assert_array_equal(o["plan"][t], acts[first[t]])
                assert int(o["n_actions"][t]) == int(nact[first[t]])
            else:
                assert np.isfinite(cost[env == t]).all()
        assert len({tuple(a.ravel()) for a in acts[env == 3]}) == int(o["n_leaves"][3])  # (distinct leaves: "first" means something)


def test_root_only_trees(ctx):
    """max_nodes_ = 0: the root is the only leaf, the plan is empty, its cost og_cost's of an empty action list."""
    o, lv = ctx.plan(2, 0.0)
    assert (o["n_nodes"] == 1).all() and (o["n_leaves"] == 1).all() and (o["n_actions"] == 0).all() and np.all(o["plan"] == 0.0)
    A = ctx.cfg.max_actions
    _, cost = ctx.eng.og_cost(ctx.i32(list(range(K.N_ENVS))), torch.zeros(K.N_ENVS, A, 3, dtype=torch.float64, device=ctx.dev),
                              ctx.i32([0] * K.N_ENVS))
    same_bits(o["cost"], cost.cpu().numpy())
    same_bits(lv["cost"].cpu().numpy(), cost.cpu().numpy())


def test_deepest_leaf_at_max_actions_and_one_beyond(ctx):
    o, lv = ctx.plan(2, SMALL)
    depth = int(lv["n_actions"].max())
    assert depth >= 2
    exact = Ctx(max_actions=depth)
    try:
        o2, lv2 = check_same_bits_as_the_cost_entry(exact, 2, SMALL)
        assert int(lv2["n_actions"].max()) == depth == exact.cfg.max_actions
        same_bits(lv2["cost"].cpu().numpy(), lv["cost"].cpu().numpy())  # (the capacity is no part of the arithmetic)
        np.testing.assert_array_equal(o2["nodes"], o["nodes"])
    finally:
        exact.eng.close()
    short = Ctx(max_actions=depth - 1)
    try:
        before = short.state()
        short.eng.set_sampler_parameter(SMALL)
        for alg in (2, 3):
            assert raw_og_plan(short, list(range(K.N_ENVS)), alg, K.ALPHA)[0] == DRLGX_E_CAPACITY
        assert short.eng.status() == 0
        for a, b in zip(before, short.state()):
            np.testing.assert_array_equal(a, b)
    finally:
        short.eng.close()


def test_a_non_monotonic_subset(ctx):
    full, _ = ctx.plan(2, SMALL)
    o, lv = ctx.plan(2, SMALL, sel=[2, 0])
    same_bits(lv["cost"].cpu().numpy(), ctx.recost(lv, 2))
    for k, v in o.items():
        np.testing.assert_array_equal(v, full[k][[2, 0]], err_msg=k)
    assert lv["cand_env"].cpu().numpy().tolist() == [2] * int(o["n_leaves"][0]) + [0] * int(o["n_leaves"][1])


@pytest.mark.parametrize("alg", [2, 3])
def test_more_than_128_leaves(ctx, alg):
    """Algorithm 3 crosses an fm2 chunk boundary (chunks of 128 candidates)."""
    o, lv = check_same_bits_as_the_cost_entry(ctx, alg, BIG)
    assert int(o["n_leaves"].sum()) >= 129 and (o["result"] == SUCCESS).all()


def raw_og_plan(c, sel, alg, alpha, sentinel=-7.0):
    """drlgx_og_plan's return code and its outputs, which start at a sentinel."""
    n, A, dev = len(sel), c.cfg.max_actions, c.dev
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    f = [torch.full((n, A, 3), sentinel, dtype=torch.float64, device=dev), torch.full((n,), sentinel, dtype=torch.float64, device=dev)]
    i = [torch.full((n,), int(sentinel), dtype=torch.int32, device=dev) for _ in range(5)]
    env_sel, start = c.i32(sel), c.i32([K.START_INDICES[e] for e in sel])  # (named: alive until the call has run)
    rc = c.eng.L.drlgx_og_plan(c.eng.h, n, p(env_sel), p(start), K.CAP, alg, alpha, p(f[0]), p(i[0]), p(f[1]), p(i[1]), p(i[2]), p(i[3]),
                               None, p(i[4]))
    torch.cuda.synchronize(dev)
    return rc, f + i


def test_refusals(ctx):
    eng = ctx.eng
    before = ctx.state()
    eng.set_sampler_parameter(SMALL)
    sel = list(range(K.N_ENVS))
    calls = [(0, K.ALPHA), (1, K.ALPHA), (4, K.ALPHA), (-1, K.ALPHA), (3, -0.1), (3, 1.5), (3, float("nan"))]
    for alg, alpha in calls:
        rc, outs = raw_og_plan(ctx, sel, alg, alpha)
        assert rc == DRLGX_E_INVALID, (alg, alpha)
        assert all(bool((t == -7).all()) for t in outs), (alg, alpha)
    eng.set_sampler_parameter(SMALL, 0.0, True)  # the Dubins flag
    try:
        for alg in (2, 3):
            rc, outs = raw_og_plan(ctx, sel, alg, K.ALPHA)
            assert rc == DRLGX_E_INVALID and all(bool((t == -7).all()) for t in outs)
    finally:
        eng.set_sampler_parameter(SMALL)
    assert raw_og_plan(ctx, sel, 2, 7.0)[0] == 0  # alpha is read under algorithm 3 only
    # drlgx_em_plan still has two algorithms
    n, A = K.N_ENVS, ctx.cfg.max_actions
    plan, nact = torch.empty(n, A, 3, dtype=torch.float64, device=ctx.dev), torch.empty(n, dtype=torch.int32, device=ctx.dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    env_sel, start = ctx.i32(sel), ctx.i32(K.START_INDICES)
    for alg in (2, 3):
        assert eng.L.drlgx_em_plan(eng.h, n, p(env_sel), p(start), K.CAP, alg, p(plan), p(nact), None, None, None, None, None,
                                   None) == DRLGX_E_INVALID
    assert eng.status() == 0
    for a, b in zip(before, ctx.state()):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("alg", [2, 3])
def test_under_the_samplers_obstacle_logic(ctx, alg):
    """safe_distance 1.5 (tests/em_safe_cases.py's) around 8 landmarks refuses about one sample in twenty: over the ~120 samples of
    the two grown trees the tree is another one than without the logic."""
    sd = em_safe_cases.SAFE_DISTANCE
    ctx.eng.set_sampler_obstacles(True)
    try:
        o = check_same_tree(ctx, MID, sd)
        check_same_bits_as_the_cost_entry(ctx, alg, MID, sd)
        plain, _ = ctx.plan(2, MID)
        assert not np.array_equal(o["halton_next"], plain["halton_next"]) or not np.array_equal(o["nodes"], plain["nodes"])
    finally:
        ctx.eng.set_sampler_obstacles(False)
        ctx.eng.set_sampler_parameter(SMALL)
