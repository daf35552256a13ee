"""GPU tests (run with -m gpu on an MI355X) of drlgx_slam_og_cost where its loops start a second trip, at the cap of 256 predicted
measurements and where its chunks of 128 candidates share the engine's own landmark buffer - k_fm2_prior_ordered and
k_fm2_update<., true> (csrc/k_fm2.hip), k_slam_og_weights and k_slam_og_blend (csrc/k_og.hip) - against tests/slam_og_ref.py on
the cases of tests/slam_og_wrap_cases.py (whose counts, margins and sensitivities tests/test_slam_og_wrap_cpu.py checks on the CPU).

What wraps.  The corridor: P + L = 280 > 256 owners in k_fm2_prior_ordered (a thread's second owner is a landmark slot >= 246),
L = 270 > 256 slots in the ordered compaction of k_fm2_update and in k_slam_og_weights, five trips per lane in k_slam_og_blend.
The rings: nm == 256 for the landmark blocks, and n_cand > 128 without lm_cov_out, so that every chunk writes the same buffer.

Tolerances: those of tests/test_gpu_slam_og.py (slam_og_check.check_case), unchanged; the bounds on sums of entropy terms (H_leaf,
w2) are argued per term at 900 cells and scaled by V / 900 for these maps of 1600 cells.

Observed on the MI355X: landmark blocks at most 4.5e-5 of their tolerance (corridor_back; 7.1e-7 at nm == 256), slam_uncertainty at
most 4.8e-6 of its bound, H_leaf within 2.3e-16, w1 of the corridor 2.6e-12 off the restatement's and 0 off numpy's on the live
marginals; every bit-for-bit comparison holds.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fm2_cases as F  # noqa: E402
import og_ref  # noqa: E402
import slam_og_cases as K  # noqa: E402
import slam_og_ref as R  # noqa: E402
import slam_og_wrap_cases as W  # noqa: E402
from slam_og_check import SUM_RTOL, bits as _bits, check_case, check_nothing_else_moved  # noqa: E402
from test_gpu_slam_og import DRLGX_E_CAPACITY, Ctx, _raw  # noqa: E402

KEYS = ("unc", "cost", "terms", "weights", "lm_cov")
_ALL = [(w, c) for w in sorted(W.CASES) for c in sorted(W.CASES[w])]
RING_STRIDE = 2   # coprime to the nine ring cases, and 128 * 2 is no multiple of 9: candidates i and i + 128 differ


class WrapCtx(Ctx):
    """test_gpu_slam_og.Ctx on a world of tests/fm2_cases.py: its oracles, its engine stepped beside them, the solo call once."""

    def __init__(self, wname):
        self.world = W.world(wname)
        self.sims = self.world.sims
        self.cases = W.CASES[wname]
        self.names = sorted(self.cases)
        self.eng, self.cfg = F.make_engine(self.world)
        self.A, self.Lmax = self.cfg.max_actions, self.cfg.max_landmarks
        self.sum_rtol = SUM_RTOL * (self.eng.rows * self.eng.cols) / 900.0
        self._ref, self._solo = {}, None

    def ref(self, name):
        if name not in self._ref:
            self._ref[name] = W.reference(self.world, name)
        return self._ref[name]

    def run(self, cases, masked=None, lm_cov=True):
        """dict of host arrays: unc, cost, terms, weights and (lm_cov) the landmark blocks; without lm_cov the call leaves the
        blocks in the engine's own chunk buffer, as the production callers do."""
        ce, acts, nact, core = self.candidates(cases, masked)
        out = self.eng.slam_og_cost(ce, acts, nact, W.ALPHA, core=core, want_terms=True, want_lm_cov=lm_cov)
        assert self.eng.status() == 0
        return dict(zip(KEYS, (t.cpu().numpy() for t in out)))

    def solo(self):
        """Every named case of the world in one call that asks for the landmark blocks: computed once."""
        if self._solo is None:
            self._solo = self.run([self.cases[n] for n in self.names])
        return self._solo

    def cycled(self, n_cand):
        return [self.names[(c * RING_STRIDE) % len(self.names)] for c in range(n_cand)]


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = WrapCtx(name)
        return made[name]
    yield get
    for c in made.values():
        c.eng.close()


def _same_bits(a, b, keys, msg=""):
    for key in keys:
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg="%s %s" % (msg, key))


@pytest.mark.parametrize("wname,name", _ALL, ids=[c for _, c in _ALL])
def test_parity_at_the_wraps(ctxs, wname, name):
    """One call per world holds all its cases.  Corridor: 10 + 270 = 280 > 256 owners of the ordered prior, 270 > 256 slots, a
    masked candidate (130 measurements from 2 of 9 poses) beside unmasked ones, so the call runs k_fm2_update<true, true>.
    Rings: nm == 256 on a fresh (P = 1) and a walked (P = 7) belief, 130, 33 | 32, 17 | 16, 0."""
    ctx = ctxs(wname)
    e, _, _, nm = ctx.cases[name]
    P, L = ctx.sims[e].num_poses(), ctx.sims[e].num_landmarks()
    if wname == "corridor":
        assert P + L == 280 > 256 and L == 270 > 256 and P == ctx.cfg.max_poses
    if name in W.AT_THE_CAP:
        assert nm == 256 == W.MAX_MEAS
    assert ctx.eng.rows * ctx.eng.cols == 1600
    ref = ctx.ref(name)
    assert ref["nm"] == nm
    check_case(ctx.sims[e], e, name, ref, ctx.solo(), ctx.names.index(name), sum_rtol=ctx.sum_rtol)


@pytest.mark.parametrize("wname", sorted(W.CASES))
def test_h_leaf_is_og_costs_entropy(ctxs, wname):
    ctx = ctxs(wname)
    ce, acts, nact, _ = ctx.candidates([ctx.cases[n] for n in ctx.names])
    ent, cost = ctx.eng.og_cost(ce, acts, nact)
    out = ctx.solo()
    np.testing.assert_array_equal(_bits(out["terms"][:, 0]), _bits(ent.cpu().numpy()))
    d_og, d_sog = cost.cpu().numpy() - ent.cpu().numpy(), out["cost"] - out["unc"]
    np.testing.assert_allclose(d_sog, d_og, rtol=0, atol=4e-16 * np.abs(cost.cpu().numpy()).max())


@pytest.mark.parametrize("wname", sorted(W.CASES))
def test_weights_from_the_live_belief(ctxs, wname):
    """w1 / w2 against numpy on Engine.landmarks() / Engine.virtual_map() - the corridor: 270 > 256 landmarks, the second trip of
    k_slam_og_weights - and, in the K = 0 cases, w1 * slam_uncertainty = alpha: the ordered dense prior against the live marginals."""
    ctx = ctxs(wname)
    out = ctx.solo()
    if wname == "corridor":
        assert ctx.eng.counts(0)["landmarks"] == 270 > 256
    for e in range(len(ctx.sims)):
        info = ctx.eng.landmarks(e)[2].reshape(-1, 2, 2)
        h = og_ref.entropy(ctx.eng.virtual_map(e)[0].reshape(-1))
        assert out["weights"][e, 1] == pytest.approx((1.0 - W.ALPHA) / h, rel=ctx.sum_rtol)
        kappa = max((m[0, 0] * m[1, 1] + m[0, 1] ** 2) / (m[0, 0] * m[1, 1] - m[0, 1] ** 2) for m in info)
        s = R.sum_sqrt_det([np.linalg.inv(m) for m in info])
        print("%s env %d: L %d  kappa %.3g  w1 %.3e off numpy's" % (wname, e, len(info), kappa, abs(out["weights"][e, 0] * s / W.ALPHA - 1)))
        assert out["weights"][e, 0] == pytest.approx(W.ALPHA / s, rel=64 * kappa * 2.0 ** -52)
    for name in [n for n in ctx.names if n.endswith("_K0")]:
        e, i = ctx.cases[name][0], ctx.names.index(name)
        root_cov = [np.linalg.inv(m) for m in ctx.sims[e].landmarks()[2]]
        rel = 2 * K.sqrt_det_sum_tol(root_cov) / R.sum_sqrt_det(root_cov)
        assert out["weights"][e, 0] * out["terms"][i, 1] == pytest.approx(W.ALPHA, rel=rel), name


def test_no_measurement_at_270_landmarks(ctxs):
    """An action that sees nothing gives the bits of the K = 0 candidate of the same call: the prior's blocks, all 270."""
    ctx = ctxs("corridor")
    out = ctx.solo()
    k0, blind = ctx.names.index("corridor_K0"), ctx.names.index("corridor_blind")
    assert ctx.ref("corridor_blind")["nm"] == 0 and len(ctx.cases["corridor_blind"][1]) == 1
    assert np.isfinite(out["lm_cov"][k0][:270]).all()
    np.testing.assert_array_equal(_bits(out["lm_cov"][blind]), _bits(out["lm_cov"][k0]))
    assert out["terms"][blind, 1] == out["terms"][k0, 1]


@pytest.mark.parametrize("wname", sorted(W.CASES))
def test_without_a_mask_the_same_bits(ctxs, wname):
    """The unmasked cases in a call without a core mask (k_fm2_update<false, true>: at L = 270 > 256, at nm == 256) and in a call
    with one (<true, true>; the corridor's solo call has a masked candidate, the rings' has not): the same bits."""
    ctx = ctxs(wname)
    names = [n for n in ctx.names if ctx.cases[n][2] is None]
    bare = ctx.run([ctx.cases[n] for n in names])
    ones = ctx.run([ctx.cases[n] for n in names], masked=True)
    _same_bits(ones, bare, KEYS, wname)
    solo = ctx.solo()
    for c, n in enumerate(names):
        for key in ("unc", "cost", "terms", "lm_cov"):
            np.testing.assert_array_equal(_bits(bare[key][c]), _bits(solo[key][ctx.names.index(n)]), err_msg="%s %s" % (n, key))


@pytest.mark.parametrize("n_cand", [128, 129, 257])
def test_the_engines_chunk_buffer(ctxs, n_cand):
    """n_cand = 128, 129, 257 > 128 WITHOUT lm_cov_out, the call of Engine.slam_og_cost's production callers: every chunk of 128
    writes its landmark blocks to the start of the engine's own buffer and the blend reads them there.  The candidates at i and
    i + 128 differ, so a chunk that read another chunk's blocks would show.  Every candidate has the bits of its twin in the solo
    call (which passed lm_cov_out); then the same call with lm_cov_out, its blocks compared as well."""
    ctx = ctxs("rings")
    order = ctx.cycled(n_cand)
    for i in range(n_cand - 128):
        a, b = ctx.cases[order[i]], ctx.cases[order[i + 128]]
        assert a[0] != b[0] or a[1] != b[1], i
    assert len({ctx.cases[n][0] for n in order[:9]}) == 6 and -(-n_cand // 128) == {128: 1, 129: 2, 257: 3}[n_cand]
    solo = ctx.solo()
    plain = ctx.run([ctx.cases[n] for n in order], lm_cov=False)
    assert sorted(plain) == ["cost", "terms", "unc", "weights"]
    full = ctx.run([ctx.cases[n] for n in order])
    for c, n in enumerate(order):
        i = ctx.names.index(n)
        for key in ("unc", "cost", "terms"):
            np.testing.assert_array_equal(_bits(plain[key][c]), _bits(solo[key][i]), err_msg="no lm_cov: candidate %d (%s) %s" % (c, n, key))
        for key in ("unc", "cost", "terms", "lm_cov"):
            np.testing.assert_array_equal(_bits(full[key][c]), _bits(solo[key][i]), err_msg="lm_cov: candidate %d (%s) %s" % (c, n, key))
    np.testing.assert_array_equal(_bits(plain["weights"]), _bits(solo["weights"]))
    np.testing.assert_array_equal(_bits(full["weights"]), _bits(solo["weights"]))


def test_the_same_call_twice_gives_the_same_bits(ctxs):
    """The corridor call (280 > 256 owners of the ordered prior) and 130 > 128 cycled ring candidates, each run twice."""
    ctx = ctxs("corridor")
    _same_bits(ctx.run([ctx.cases[n] for n in ctx.names]), ctx.solo(), KEYS, "corridor")
    ctx = ctxs("rings")
    order = ctx.cycled(130)
    a, b = ctx.run([ctx.cases[n] for n in order]), ctx.run([ctx.cases[n] for n in order])
    _same_bits(a, b, KEYS, "rings")
    a, b = ctx.run([ctx.cases[n] for n in order], lm_cov=False), ctx.run([ctx.cases[n] for n in order], lm_cov=False)
    _same_bits(a, b, ("unc", "cost", "terms", "weights"), "rings without lm_cov")


@pytest.mark.parametrize("wname,served", [("corridor", ("corridor_end", "corridor_back")), ("rings", ("fresh_K8", "walked_K8"))])
def test_over_the_cap_between_two_served(ctxs, wname, served):
    """More than 256 predicted measurements (the corridor's 326, the ring's 288) between two served candidates: DRLGX_E_CAPACITY,
    the outputs and the status word untouched."""
    ctx = ctxs(wname)
    eng, dev = ctx.eng, ctx.eng.device
    e, plan, core = W.OVERFLOWS[wname]
    assert W.predicted(ctx.sims[e], plan, core) > W.MAX_MEAS
    ce, acts, nact, _ = ctx.candidates([ctx.cases[served[0]], (e, plan, core, None), ctx.cases[served[1]]])
    unc = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    cost = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    lm = torch.full((3, ctx.Lmax, 3), -7.0, dtype=torch.float64, device=dev)
    eng.use_torch_stream()
    assert _raw(eng, ce, acts, nact, W.ALPHA, unc, cost, lm=lm) == DRLGX_E_CAPACITY
    assert _raw(eng, ce, acts, nact, W.ALPHA, unc, cost) == DRLGX_E_CAPACITY
    assert eng.status() == 0
    assert bool((unc == -7.0).all()) and bool((cost == -7.0).all()) and bool((lm == -7.0).all())


def test_a_mask_brings_the_overflow_under_the_cap(ctxs):
    """The corridor's overflow plan with two of its four poses masked out predicts 166 <= 256: served between the same two
    neighbours, held to the restatement like any case; the neighbours keep their bits."""
    ctx = ctxs("corridor")
    e, plan, core, nm = W.MASKED_OVERFLOW
    assert W.predicted(ctx.sims[e], plan, None) > W.MAX_MEAS >= W.predicted(ctx.sims[e], plan, core) == nm > 0
    out = ctx.run([ctx.cases["corridor_end"], W.MASKED_OVERFLOW, ctx.cases["corridor_back"]])
    ref = W.reference(ctx.world, W.MASKED_OVERFLOW)
    assert ref["nm"] == nm
    check_case(ctx.sims[e], e, "masked overflow", ref, out, 1, sum_rtol=ctx.sum_rtol)
    solo = ctx.solo()
    for c, n in ((0, "corridor_end"), (2, "corridor_back")):
        for key in ("unc", "cost", "terms", "lm_cov"):
            np.testing.assert_array_equal(_bits(out[key][c]), _bits(solo[key][ctx.names.index(n)]), err_msg="%s %s" % (n, key))


def test_nothing_else_moved(ctxs):
    """slam_og_check.check_nothing_else_moved on the corridor, around a call with and a call without lm_cov_out: the getters
    return the same bits; drlgx_fm2_update_steps / drlgx_em_cost_steps the same bits where their own calls repeat theirs, and
    otherwise what tests/test_gpu_fm2.py holds them to (the update term within 10 x its C4 spread)."""
    ctx = ctxs("corridor")
    cases = [ctx.cases[n] for n in ctx.names]
    bound = {n: F.DELTA_BOUND_FACTOR * F.C4_DELTA_SPREAD[n] for n in ("corridor_end", "corridor_back")}
    check_nothing_else_moved(ctx, ctx.names, cases, [lambda: ctx.run(cases), lambda: ctx.run(cases, lm_cov=False)],
                             ["corridor_K0", "corridor_end", "corridor_back"], "corridor_back", delta_bound=bound)


def test_behind_a_lazy_restore(ctxs):
    """snapshot, one step of every environment, restore (lazy: DRLGX_RESTORE_EAGER is not set), and the call is the first to enter
    the engine: the same bits in every output as before the snapshot, with and without lm_cov_out; a step after it leaves the
    status word 0.  A last restore hands the engine back as it was."""
    ctx = ctxs("rings")
    eng = ctx.eng
    cases = [ctx.cases[n] for n in ctx.cycled(130)]
    before, before_plain = ctx.run(cases), ctx.run(cases, lm_cov=False)
    live = lambda: [[eng.counts(e)[k] for k in ("poses", "landmarks", "factors")] for e in range(len(ctx.sims))]  # noqa: E731
    counts = live()
    odom = torch.tensor([F.RING_SHORT] * len(ctx.sims), dtype=torch.float64, device=eng.device)
    eng.snapshot(0)
    eng.step(odom)
    assert eng.status() == 0 and [c[0] for c in live()] == [c[0] + 1 for c in counts]
    eng.restore(0)
    _same_bits(ctx.run(cases), before, KEYS, "behind the restore")
    eng.step(odom)
    assert eng.status() == 0
    eng.restore(0)
    _same_bits(ctx.run(cases, lm_cov=False), before_plain, ("unc", "cost", "terms", "weights"), "behind the second restore")
    assert eng.status() == 0 and live() == counts
    _same_bits(ctx.run([ctx.cases[n] for n in ctx.names]), ctx.solo(), KEYS, "the solo call afterwards")
