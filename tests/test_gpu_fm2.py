"""GPU tests (run with -m gpu on an MI355X) of the fm2 covariance update - k_fm2_prior / k_fm2_update (csrc/k_fm2.hip) through
drlgx_fm2_update and drlgx_em_cost - where its loops wrap and at the cap of 256 predicted measurements, against oracle/fm2_ref.py
on the beliefs and plans of tests/fm2_cases.py.  tests/test_fm2_cpu.py checks on the CPU that those cases predict the named
numbers of measurements (C1), sit on no gate (C2), would fail if the update term were dropped (C3), and how far the restatement
is from a second, information-form evaluation of itself (C4).

Tolerances.  The updated covariances Sigma': the project's rtol 1e-6 / atol 1e-10 (tests/test_gpu_belief.py), unchanged.  The
update term (cov_gpu - base_ref) against Delta_ref = Sigma'_ref - base_ref, relative to max |Delta_ref| of the candidate: 10 x the
C4 spread of Delta of that case (fm2_cases.C4_DELTA_SPREAD, measured on the CPU: 1.3e-14 at nm = 7 ... 5.5e-13 at nm = 256, so
bounds of 1.3e-13 ... 5.5e-12) - one decade for the other summation order, the fp64 atomics of k_fm2_prior and Gauss-Jordan
against LAPACK, as for DOPT_RTOL of tests/test_gpu_em.py.  Dropping the term is an error of 1 on that scale.

Observed on the MI355X: Sigma' at most 9.4e-4 of its tolerance (walked_K8); the update term 1.1e-14 (em_plan2) ... 1.1e-12
(corridor_back) of max |Delta|, at most 0.48 of its bound (ring33_K1: 1.1e-13 of 2.3e-13; nm = 256: 6.9e-13 and 9.3e-13 of
2.5e-12 and 5.5e-12).  Two calls do not return the same bits (the atomics of k_fm2_prior; up to 5e-12 relative apart), the
candidates of one call do, wherever they stand in it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_ref  # noqa: E402
import fm2_cases as F  # noqa: E402
from test_gpu_belief import compare_state  # noqa: E402
from test_gpu_em import DRLGX_E_CAPACITY, _check_against_ref, _raw_em_cost  # noqa: E402

_WORLDS = {"rings": F.rings_world, "corridor": F.corridor_world, "em_cases": F.em_world}
_ALL_CASES = [("rings", c) for c in F.RING_NM] + [("corridor", c) for c in F.CORRIDOR_PLANS] + [("em_cases", c) for c in F.EM_PLANS]


class Ctx(object):
    """One world: its oracles, its engine stepped beside them, and every candidate's solo run computed once."""

    def __init__(self, world):
        self.world = world
        self.sims = world.sims
        self.eng, self.cfg = F.make_engine(world)
        self.A, self.stride = self.cfg.max_actions, self.cfg.max_poses + self.cfg.max_actions
        self._solo = {}

    def candidates(self, plans):
        """Device arrays of a list of (environment, plan)."""
        acts = np.zeros((len(plans), self.A, 3))
        for c, (_, plan) in enumerate(plans):
            acts[c, :len(plan)] = np.reshape(plan, (-1, 3))
        dev = self.eng.device
        return (torch.tensor([e for e, _ in plans], dtype=torch.int32, device=dev), torch.tensor(acts, device=dev),
                torch.tensor([len(p) for _, p in plans], dtype=torch.int32, device=dev))

    def fm2(self, plans):
        """drlgx_fm2_update into buffers pre-filled with NaN / -1: (cov [C, stride, 3, 3], n_out [C]) on the host."""
        ce, acts, nact = self.candidates(plans)
        cov = torch.full((len(plans), self.stride, 3, 3), float("nan"), dtype=torch.float64, device=self.eng.device)
        n_out = torch.full((len(plans),), -1, dtype=torch.int32, device=self.eng.device)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        self.eng.use_torch_stream()
        assert self.eng.L.drlgx_fm2_update(self.eng.h, len(plans), p(ce), p(acts), p(nact), p(cov), self.stride, p(n_out)) == 0
        assert self.eng.status() == 0
        return cov.cpu().numpy(), n_out.cpu().numpy()

    def solo(self, case):
        if case not in self._solo:
            cov, n_out = self.fm2([self.world.plans[case]])
            self._solo[case] = (cov[0], int(n_out[0]))
        return self._solo[case]


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Ctx(_WORLDS[name]())
        return made[name]
    yield get
    for c in made.values():
        c.eng.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("wname,case", _ALL_CASES, ids=[c for _, c in _ALL_CASES])
def test_parity_and_structure(ctxs, wname, case):
    """Sigma' at the project's tolerance, the update term at 10 x the restatement's own spread, n_out exact; every block
    symmetric to the bit, no old pose's trace grown, the rows behind n_out untouched."""
    ctx = ctxs(wname)
    ref = ctx.world.ref(case)
    cov, n_out = ctx.solo(case)
    P, K = ref["P"], ref["K"]
    assert n_out == P + K == ref["cov"].shape[0]
    assert np.isnan(cov[n_out:]).all() and np.isfinite(cov[:n_out]).all()
    got = cov[:n_out]
    np.testing.assert_array_equal(_bits(got), _bits(got.transpose(0, 2, 1)))
    gap = np.abs(got - ref["cov"]) / (F.SIGMA_RTOL * np.abs(ref["cov"]) + F.SIGMA_ATOL)
    line = "%s: nm %d  Sigma' gap / tolerance %.3e" % (case, ref["nm"], gap.max())
    if ref["nm"]:
        bound = F.DELTA_BOUND_FACTOR * F.C4_DELTA_SPREAD[case]
        ratio = np.abs((got - ref["base"]) - ref["delta"]).max() / np.abs(ref["delta"]).max()
        line += "  update term: %.3e of max |Delta| (bound %.1e, the base alone %.3e)" % (
            ratio, bound, np.abs(ctx.solo(F.k0_of(case))[0][:P] - ref["base"][:P]).max() / np.abs(ref["delta"]).max())
    print(line)
    np.testing.assert_allclose(got, ref["cov"], rtol=F.SIGMA_RTOL, atol=F.SIGMA_ATOL, err_msg=case)
    # old poses: the update only ever removes uncertainty (against the engine's own prior blocks: the K = 0 run, bit for bit
    # the base the kernel subtracts from when the two runs' priors are the same bits)
    prior = ctx.solo(F.k0_of(case))[0][:P]
    for i in range(P):
        assert np.trace(got[i]) <= np.trace(prior[i]) * (1 + 1e-9), (case, i)
    if ref["nm"] == 0:
        np.testing.assert_allclose(got, ref["base"], rtol=F.SIGMA_RTOL, atol=F.SIGMA_ATOL)
    else:
        assert case in F.PARITY_CASES and 100 * bound < 1.0
        assert ratio <= bound, "%s: update term off by %.3e of max |Delta|, bound %.1e" % (case, ratio, bound)


def test_at_the_cap(ctxs):
    """nm = 256 is served (status 0; its parity is test_parity_and_structure's); one action more on the ring (288) and the
    corridor's overflow plan make drlgx_em_cost return DRLGX_E_CAPACITY with the outputs and the status word untouched."""
    for wname, full, over in (("rings", "walked_K8", F.RING_OVERFLOW), ("corridor", "corridor_back", F.CORRIDOR_OVERFLOW)):
        ctx = ctxs(wname)
        dev = ctx.eng.device
        assert ctx.world.ref(full)["nm"] <= F.MAX_MEAS < F.reference(ctx.sims[over[0]], over[1])["nm"]
        for alg in (0, 1):
            ce, acts, nact = ctx.candidates([ctx.world.plans[full], over, ctx.world.plans[full]])
            unc = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
            cost = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
            assert _raw_em_cost(ctx.eng, ce, acts, nact, alg, unc, cost) == DRLGX_E_CAPACITY
            assert ctx.eng.status() == 0
            assert bool((unc == -7.0).all()) and bool((cost == -7.0).all())
            ce, acts, nact = ctx.candidates([ctx.world.plans[full]] * 3)
            assert _raw_em_cost(ctx.eng, ce, acts, nact, alg, unc, cost) == 0
            assert ctx.eng.status() == 0 and float(unc.min()) > 0 and float(cost.min()) > 0
    assert ctxs("rings").world.ref("walked_K8")["nm"] == ctxs("rings").world.ref("fresh_K8")["nm"] == F.MAX_MEAS


def test_mixed_launches(ctxs):
    """One call of 135 candidates - more than one chunk of 128 - that interleaves nm = 256, no sighting, 65, 17 and no action,
    from four environments: the same candidate gets the same bits wherever it stands in the launch (any block, either chunk:
    the scratch layout), the reversed order gives the same bits, and each equals its solo run.

    k_fm2_prior sums with fp64 atomics, so two CALLS need not see the same prior bits.  Within one call every candidate of an
    environment reads one prior, so the first two checks are unconditional; the comparison across calls is bit for bit only when two
    solo runs of every candidate are themselves bit-equal.  Observed on the MI355X: they are not (the outputs of two calls
    differ by up to 5e-12 relative), so there the mixed and the reversed launch are held to the restatement with the bounds of
    test_parity_and_structure instead."""
    ctx = ctxs("rings")
    names = ["walked_K8", "walked_blind", "ring65_K1", "ring17_K1", "fresh_K0"]
    assert [ctx.world.ref(n)["nm"] for n in names] == [256, 0, 65, 17, 0] and ctx.world.ref("fresh_K0")["K"] == 0
    order = [names[c % 5] for c in range(135)]
    cov, n_out = ctx.fm2([ctx.world.plans[n] for n in order])
    rcov, rn_out = ctx.fm2([ctx.world.plans[n] for n in reversed(order)])
    rcov, rn_out = rcov[::-1], rn_out[::-1]
    first = {n: order.index(n) for n in names}
    for c, n in enumerate(order):
        assert n_out[c] == n_out[first[n]] == rn_out[c]
        np.testing.assert_array_equal(_bits(cov[c]), _bits(cov[first[n]]), err_msg="candidate %d (%s)" % (c, n))   # NaN rows too
        np.testing.assert_array_equal(_bits(rcov[c]), _bits(rcov[first[n]]), err_msg="reversed candidate %d (%s)" % (c, n))
    assert order[128] != order[127] and 134 // 128 == 1
    again = {n: ctx.fm2([ctx.world.plans[n]]) for n in names}
    stable = all(np.array_equal(_bits(again[n][0][0]), _bits(ctx.solo(n)[0])) for n in names)
    print("two solo runs of every candidate bit-equal: %s" % stable)
    for n in names:
        solo, solo_n = ctx.solo(n)
        assert solo_n == n_out[first[n]]
        for other, tag in ((cov[first[n]], "mixed"), (rcov[first[n]], "reversed")):
            if stable:
                np.testing.assert_array_equal(_bits(other), _bits(solo), err_msg="%s %s vs solo" % (n, tag))
            else:  # another call, another prior: held to the restatement exactly as the solo run is
                ref = ctx.world.ref(n)
                assert np.isnan(other[solo_n:]).all()
                np.testing.assert_allclose(other[:solo_n], ref["cov"], rtol=F.SIGMA_RTOL, atol=F.SIGMA_ATOL, err_msg="%s %s" % (n, tag))
                if ref["nm"]:
                    ratio = np.abs((other[:solo_n] - ref["base"]) - ref["delta"]).max() / np.abs(ref["delta"]).max()
                    print("%s %s: update term %.3e of max |Delta|" % (n, tag, ratio))
                    assert ratio <= F.DELTA_BOUND_FACTOR * F.C4_DELTA_SPREAD[n], (n, tag, ratio)


class _EmRef(object):
    """What test_gpu_em._check_against_ref reads: the oracles and em_ref's result of a case."""

    def __init__(self, ctx):
        self.sims, self.world, self._ref = ctx.sims, ctx.world, {}

    def ref(self, e, case):
        if case not in self._ref:
            self._ref[case] = em_ref.em_costs(self.sims[e], self.world.plans[case][1], cov=self.world.ref(case)["cov"])
        return self._ref[case]


@pytest.mark.parametrize("wname,case", F.EM_COST_CASES, ids=[c for _, c in F.EM_COST_CASES])
def test_em_cost_on_the_dense_cases(ctxs, wname, case):
    """drlgx_em_cost, both algorithms, against tests/em_ref.py at the tolerances of tests/test_gpu_em.py; which cells stay at
    I / sigma0^2 must agree exactly."""
    ctx = ctxs(wname)
    e, plan = ctx.world.plans[case]
    ce, acts, nact = ctx.candidates([(e, plan)])
    unc0, cost0, info = ctx.eng.em_cost(ce, acts, nact, 0, want_info=True)
    unc1, cost1 = ctx.eng.em_cost(ce, acts, nact, 1)
    assert ctx.eng.status() == 0
    ref = _EmRef(ctx)
    assert min(ref.ref(e, case)[3].values()) > 1e-9
    _check_against_ref(ref, e, case, float(unc0[0]), float(cost0[0]), float(unc1[0]), float(cost1[0]), info[0].cpu().numpy(), case)


def test_live_state_is_untouched(ctxs):
    """Last: after every call above the environments still are their oracles'."""
    for wname in _WORLDS:
        ctx = ctxs(wname)
        for i, sim in enumerate(ctx.sims):
            compare_state(ctx.eng, i, sim, "%s env %d after the fm2 tests" % (wname, i))
