"""GPU tests (run with -m gpu on an MI355X) of the SLAM-OG-Shannon cost of candidate plans - drlgx_slam_og_cost: the landmark blocks
of k_fm2_update (csrc/k_fm2.hip), the root weights and the blend (csrc/k_og.hip) - against tests/slam_og_ref.py on the world of
tests/slam_og_cases.py (whose counts, margins and closed forms tests/test_slam_og_cpu.py checks on the CPU).

Tolerances.
  * Landmark blocks Sigma'(l, l): rtol 1e-6 / atol 1e-10, what tests/test_gpu_fm2.py holds the pose blocks to, unchanged.
  * H_leaf: drlgx_og_cost's bits for the same candidates (the same kernel); against og_ref rel 1e-12 (tests/test_gpu_og.py's bound:
    900 terms of at most ln 2, each within a few ulp, another order).
  * slam_uncertainty: what an element-wise move of the blocks by 1e-6 can do to sum sqrt(det) (slam_og_cases.sqrt_det_sum_tol, from
    the reference's blocks).
  * w1 / w2 against numpy on Engine.landmarks() / Engine.virtual_map(): w2 rel 1e-12 (as H_leaf); w1 rel 64 kappa 2^-52 with
    kappa = max_l (a d + b^2) / (a d - b^2) of the information blocks - the determinant's cancellation times a few roundings of
    another order of operations.
  * uncertainty, cost: bit-equal to w2 H_leaf + w1 slam_uncertainty evaluated in numpy from the call's own terms and weights (the
    blend is compiled without contraction); against the reference the sum of the terms' bounds above, the root's sum held to 1e-6
    like the leaf's.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import og_ref  # noqa: E402
import slam_og_cases as K  # noqa: E402
import slam_og_ref as R  # noqa: E402
from slam_og_check import SUM_RTOL, bits as _bits, check_case, check_nothing_else_moved  # noqa: E402

DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3
NAMES = sorted(K.CASES)


class Ctx(object):
    def __init__(self):
        self.world = K.world()
        self.sims = self.world.sims
        self.eng, self.cfg = K.make_engine(self.world)
        self.A, self.Lmax = self.cfg.max_actions, self.cfg.max_landmarks
        self._ref, self._solo = {}, None

    def ref(self, name):
        if name not in self._ref:
            self._ref[name] = K.reference(self.world, name)
        return self._ref[name]

    def candidates(self, cases, masked=None):
        """Device arrays of a list of (environment, plan, core, nm); the core mask only if a case has one (or `masked`)."""
        acts = np.zeros((len(cases), self.A, 3))
        core = np.ones((len(cases), self.A), dtype=np.uint8)
        for c, (_, plan, mask, _) in enumerate(cases):
            acts[c, :len(plan)] = np.reshape(plan, (-1, 3))
            if mask is not None:
                core[c, :len(mask)] = mask
        dev = self.eng.device
        use = any(m is not None for _, _, m, _ in cases) if masked is None else masked
        return (torch.tensor([e for e, _, _, _ in cases], dtype=torch.int32, device=dev), torch.tensor(acts, device=dev),
                torch.tensor([len(p) for _, p, _, _ in cases], dtype=torch.int32, device=dev),
                torch.tensor(core, device=dev) if use else None)

    def run(self, cases, alpha=K.ALPHA, distance=None, masked=None):
        """dict of host arrays: unc, cost, terms, weights, lm_cov."""
        ce, acts, nact, core = self.candidates(cases, masked)
        out = self.eng.slam_og_cost(ce, acts, nact, alpha, core=core, distance=distance, want_terms=True, want_lm_cov=True)
        assert self.eng.status() == 0
        return dict(zip(("unc", "cost", "terms", "weights", "lm_cov"), (t.cpu().numpy() for t in out)))

    def solo(self):
        """Every named case, one call each way it can stand alone: computed once."""
        if self._solo is None:
            self._solo = self.run([K.CASES[n] for n in NAMES])
        return self._solo


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.eng.close()


def _check_case(ctx, name, out, i, distance=None):
    """slam_og_check.check_case (shared with tests/test_gpu_slam_og_wrap.py) on a named case of this world."""
    ref = ctx.ref(name) if distance is None else K.reference(ctx.world, name, distance=distance)
    e = K.CASES[name][0]
    check_case(ctx.sims[e], e, name, ref, out, i, sum_rtol=SUM_RTOL)


@pytest.mark.parametrize("name", NAMES)
def test_blocks_terms_and_cost_against_the_restatement(ctx, name):
    """70 landmarks (more than the blend's 64 lanes, the update's 4 waves), 24; nm = 0 ... 216; n_actions = 0, 1, max_actions; the
    core mask.  One call holds all cases: environments interleaved, masked and unmasked candidates side by side."""
    assert ctx.sims[0].num_landmarks() == 70 > 64
    _check_case(ctx, name, ctx.solo(), NAMES.index(name))


def test_h_leaf_is_og_costs_entropy(ctx):
    cases = [K.CASES[n] for n in NAMES]
    ce, acts, nact, _ = ctx.candidates(cases)
    ent, cost = ctx.eng.og_cost(ce, acts, nact)
    out = ctx.solo()
    np.testing.assert_array_equal(_bits(out["terms"][:, 0]), _bits(ent.cpu().numpy()))
    # the cost's second term is og_cost's: distance * distance_weight
    d_og, d_sog = cost.cpu().numpy() - ent.cpu().numpy(), out["cost"] - out["unc"]
    np.testing.assert_allclose(d_sog, d_og, rtol=0, atol=4e-16 * np.abs(cost.cpu().numpy()).max())


def test_weights_from_the_live_belief(ctx):
    """w1 / w2 from Engine.landmarks() and Engine.virtual_map(); the environment without a landmark: w1 = inf, NaN uncertainty."""
    out = ctx.run([K.CASES["big_K1"], (K.BLIND_ENV, [K.SHORT], None, 0), K.CASES["walked_K1"]])
    for e in range(K.N_ENVS):
        info = ctx.eng.landmarks(e)[2].reshape(-1, 2, 2)
        prob = ctx.eng.virtual_map(e)[0].reshape(-1)
        h = og_ref.entropy(prob)
        assert out["weights"][e, 1] == pytest.approx((1.0 - K.ALPHA) / h, rel=SUM_RTOL)
        if e == K.BLIND_ENV:
            assert len(info) == 0 and out["weights"][e, 0] == math.inf
            continue
        kappa = max((m[0, 0] * m[1, 1] + m[0, 1] ** 2) / (m[0, 0] * m[1, 1] - m[0, 1] ** 2) for m in info)
        s = R.sum_sqrt_det([np.linalg.inv(m) for m in info])
        print("env %d: kappa %.3g  w1 %.3e off numpy's" % (e, kappa, abs(out["weights"][e, 0] * s / K.ALPHA - 1)))
        assert out["weights"][e, 0] == pytest.approx(K.ALPHA / s, rel=64 * kappa * 2.0 ** -52)
    assert math.isnan(out["unc"][1]) and math.isnan(out["cost"][1])  # inf * 0: documented, not special-cased
    assert np.isfinite(out["unc"][[0, 2]]).all() and np.isnan(out["lm_cov"][1]).all() and out["terms"][1, 1] == 0.0
    assert ctx.eng.status() == 0


def test_no_measurement_leaves_the_prior_blocks(ctx):
    """nm = 0 - no action, and an action that sees nothing - gives the bits of the blocks that the K = 0 candidate of the same
    call has (the prior's), and w1 * slam_uncertainty = alpha up to the live marginals' tolerance."""
    out = ctx.solo()
    k0, blind = NAMES.index("walked_K0"), NAMES.index("walked_blind")
    np.testing.assert_array_equal(_bits(out["lm_cov"][blind]), _bits(out["lm_cov"][k0]))
    assert out["terms"][blind, 1] == out["terms"][k0, 1]
    for i, e in ((k0, 1), (NAMES.index("big_K0"), 0)):
        root_cov = [np.linalg.inv(m) for m in ctx.sims[e].landmarks()[2]]
        rel = 2 * K.sqrt_det_sum_tol(root_cov) / R.sum_sqrt_det(root_cov)
        assert out["weights"][e, 0] * out["terms"][i, 1] == pytest.approx(K.ALPHA, rel=rel)


@pytest.mark.parametrize("n_cand", [1, 128, 129])
def test_candidate_counts_at_the_chunk_boundary(ctx, n_cand):
    """n_cand = 1, 128 and 129 (one chunk, one chunk and one candidate), the cases cycled so that the environments interleave:
    every candidate has the bits of its solo-call twin, whichever block or chunk it stands in."""
    order = [NAMES[(c * 4) % len(NAMES)] for c in range(n_cand)]
    out, solo = ctx.run([K.CASES[n] for n in order]), ctx.solo()
    if n_cand > 1:
        assert len({K.CASES[n][0] for n in order[:4]}) == 2
    for c, n in enumerate(order):
        i = NAMES.index(n)
        for key in ("unc", "cost", "terms", "lm_cov"):
            np.testing.assert_array_equal(_bits(out[key][c]), _bits(solo[key][i]), err_msg="candidate %d (%s) %s" % (c, n, key))
    np.testing.assert_array_equal(_bits(out["weights"]), _bits(solo["weights"]))


def test_core_mask_and_distance(ctx):
    """The masked plan without its mask predicts twice the measurements and gets other blocks; all-ones mask = no mask, bit for bit;
    a caller's distance replaces the plan's own in the cost only."""
    e, plan, core, nm = K.CASES["walked_core"]
    solo = ctx.solo()
    i = NAMES.index("walked_core")
    bare = ctx.run([(e, plan, None, 2 * nm)])
    assert np.abs(bare["lm_cov"][0] - solo["lm_cov"][i])[:24].max() > 100 * K.LM_RTOL * np.abs(solo["lm_cov"][i][:24]).max()
    ones = ctx.run([(e, plan, None, 2 * nm)], masked=True)
    for key in ("unc", "cost", "terms", "lm_cov"):
        np.testing.assert_array_equal(_bits(ones[key]), _bits(bare[key]))
    dist = torch.tensor([7.25], dtype=torch.float64, device=ctx.eng.device)
    far = ctx.run([K.CASES["walked_core"]], distance=dist)
    assert far["unc"][0] == solo["unc"][i] and far["cost"][0] != solo["cost"][i]
    _check_case(ctx, "walked_core", far, 0, distance=7.25)


def _raw(eng, ce, acts, nact, alpha, unc, cost, core=None, lm=None):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return eng.L.drlgx_slam_og_cost(eng.h, ce.numel(), p(ce), p(acts), p(nact), p(core), None, alpha, p(unc), p(cost), None, None, p(lm))


def test_over_the_cap_and_bad_arguments(ctx):
    """A candidate with 280 predicted measurements between two served ones: DRLGX_E_CAPACITY, as drlgx_em_cost returns for it, the
    outputs and the status word untouched; without it the neighbours are served with their usual bits.  NULL outputs, n_cand = 0
    and an alpha outside [0, 1] are DRLGX_E_INVALID; Engine.slam_og_cost raises for the alpha."""
    eng, dev = ctx.eng, ctx.eng.device
    assert K.OVERFLOW[3] > K.MAX_MEAS
    cases = [K.CASES["big_K3"], K.OVERFLOW, K.CASES["walked_K9"]]
    ce, acts, nact, _ = ctx.candidates(cases)
    unc = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    cost = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    lm = torch.full((3, ctx.Lmax, 3), -7.0, dtype=torch.float64, device=dev)
    eng.use_torch_stream()
    assert _raw(eng, ce, acts, nact, K.ALPHA, unc, cost, lm=lm) == DRLGX_E_CAPACITY
    assert eng.L.drlgx_em_cost(eng.h, 3, C.c_void_p(ce.data_ptr()), C.c_void_p(acts.data_ptr()), C.c_void_p(nact.data_ptr()), 0,
                               C.c_void_p(unc.data_ptr()), C.c_void_p(cost.data_ptr()), None) == DRLGX_E_CAPACITY
    assert eng.status() == 0
    assert bool((unc == -7.0).all()) and bool((cost == -7.0).all()) and bool((lm == -7.0).all())
    for bad in (-0.01, 1.01, float("nan")):
        assert _raw(eng, ce[:1], acts[:1], nact[:1], bad, unc, cost) == DRLGX_E_INVALID
    assert _raw(eng, ce[:0], acts[:0], nact[:0], K.ALPHA, unc, cost) == DRLGX_E_INVALID
    assert _raw(eng, ce[:1], acts[:1], nact[:1], K.ALPHA, None, cost) == DRLGX_E_INVALID
    assert _raw(eng, ce[:1], acts[:1], nact[:1], K.ALPHA, unc, None) == DRLGX_E_INVALID
    assert eng.status() == 0 and bool((unc == -7.0).all()) and bool((cost == -7.0).all())
    with pytest.raises(ValueError):
        eng.slam_og_cost(ce[:1], acts[:1], nact[:1], 1.5)
    keep = [0, 2]
    idx = torch.tensor(keep, device=dev)
    assert _raw(eng, ce[idx].contiguous(), acts[idx].contiguous(), nact[idx].contiguous(), K.ALPHA, unc, cost) == 0
    solo = ctx.solo()
    got_u, got_c = unc.cpu().numpy(), cost.cpu().numpy()
    for c, n in enumerate(("big_K3", "walked_K9")):
        assert got_u[c] == solo["unc"][NAMES.index(n)] and got_c[c] == solo["cost"][NAMES.index(n)]
    assert got_u[2] == -7.0 and eng.status() == 0


def test_nothing_else_moved(ctx):
    """drlgx_fm2_update_steps / drlgx_em_cost_steps before and after drlgx_slam_og_cost, and the getters: the call leaves the live
    state (the same bits through the getters) and the workspaces they read alone (slam_og_check.check_nothing_else_moved: the
    same bits where those entries repeat their own, otherwise their restatements at their tests' tolerances)."""
    cases = [K.CASES[n] for n in NAMES]
    check_nothing_else_moved(ctx, NAMES, cases, [lambda: ctx.run(cases), lambda: ctx.run(cases)],
                             [n for n in NAMES if K.CASES[n][2] is None], "walked_K9")


def test_the_same_call_twice_gives_the_same_bits(ctx):
    order = [NAMES[c % len(NAMES)] for c in range(130)]
    a, b = ctx.run([K.CASES[n] for n in order]), ctx.run([K.CASES[n] for n in order])
    for key in a:
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)


def test_planner_facade_leaf_slam_entropy():
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
    ce, nact = torch.zeros(1, dtype=torch.int32, device=eng.device), torch.tensor([3], dtype=torch.int32, device=eng.device)
    alpha = ex._planner.get_parameter().alpha
    unc, cost = eng.slam_og_cost(ce, acts, nact, alpha)
    u, c = ex._planner.leaf_slam_entropy(ex._slam, ex._virtual_map, plan, return_cost=True)
    assert (u, c) == (float(unc[0]), float(cost[0])) and c > u > 0
    assert ex._planner.leaf_slam_entropy(ex._slam, ex._virtual_map, plan) == u
    eng.check_status()


def test_vec_env_rewards_from_the_slam_og_cost():
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    import em_cases
    n = 4
    env = VecExplorationEnv(em_cases.MAP, n, env_index=0, test=True, starts=em_cases.generic_starts(n), max_poses=60, n_rollouts=7)
    g = env.graph_matrix()
    actions, n_act = env.actions_all_goals()
    r, raw = env.rewards_all_goals(lookahead="slam_og", return_raw=True)
    r_og = env.rewards_all_goals(lookahead="og")
    cand_env, _, first = env.candidates
    dev = env.engine.device
    assert env.alpha == 0.5
    _, cost = env.engine.slam_og_cost(cand_env, actions, n_act, env.alpha)
    root, _ = env.engine.slam_og_cost(torch.arange(n, dtype=torch.int32, device=dev), torch.zeros(n, actions.shape[1], 3, dtype=torch.float64, device=dev),
                                      torch.zeros(n, dtype=torch.int32, device=dev), env.alpha)
    assert torch.equal(raw, root[cand_env.long()] - cost)
    assert r.shape == r_og.shape and r.dtype == r_og.dtype
    r_h, raw_h, first_h, nfr = r.cpu().numpy(), raw.cpu().numpy(), first.cpu().numpy(), g["n_frontier_h"]
    assert np.all(r_h >= -1.0) and np.all(r_h <= 1.0)
    for e in range(n):  # exploration_env.py:151-161: the arg-max goes to 0 when it is the nearest frontier, else to 1
        seg = slice(first_h[e], first_h[e] + nfr[e])
        if nfr[e] > 1 and raw_h[seg].max() > raw_h[seg].min():
            best = int(np.argmax(raw_h[seg]))
            assert r_h[seg][best] == (0.0 if best == 0 else 1.0) and r_h[seg].min() == -1.0
    with pytest.raises(ValueError):
        env.rewards_all_goals(lookahead="slam")
    env.engine.check_status()
    env.close()
