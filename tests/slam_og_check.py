"""TEST INFRASTRUCTURE: what tests/test_gpu_slam_og.py and tests/test_gpu_slam_og_wrap.py hold one candidate of a
drlgx_slam_og_cost call to, against the restatement tests/slam_og_ref.py.  The tolerances are argued in tests/test_gpu_slam_og.py.
"""
import numpy as np
import pytest

import slam_og_cases as K
import slam_og_ref as R

SUM_RTOL = 1e-12   # tests/test_gpu_og.py's bound on a sum of 900 entropy terms


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def blocks3(ref_blocks):
    return np.stack([ref_blocks[:, 0, 0], ref_blocks[:, 0, 1], ref_blocks[:, 1, 1]], axis=1)


def check_case(sim, env, name, ref, out, i, sum_rtol=SUM_RTOL):
    """Candidate `i` of the call's outputs `out` (dict of host arrays: unc, cost, terms, weights, lm_cov) against `ref`
    (slam_og_ref.slam_og_cost of the same plan on `sim`, the oracle of environment `env`).  sum_rtol: the relative bound on a sum
    of the map's entropy terms - SUM_RTOL at 900 cells, in proportion for a larger map."""
    L = sim.num_landmarks()
    got, want = out["lm_cov"][i], blocks3(ref["lm_cov"])
    gap = (np.abs(got[:L] - want) / (K.LM_RTOL * np.abs(want) + K.LM_ATOL)).max()
    s_tol = K.sqrt_det_sum_tol(ref["lm_cov"])
    root_cov = [np.linalg.inv(m) for m in sim.landmarks()[2]]
    root_rel = K.sqrt_det_sum_tol(root_cov) / R.sum_sqrt_det(root_cov)
    h, s = out["terms"][i]
    w1, w2 = out["weights"][env]
    print("%s: nm %d  blocks gap / tolerance %.3e  H_leaf %.2e  slam_uncertainty %.3e of its bound  w1 %.2e  w2 %.2e  unc %.2e  cost %.2e" % (
        name, ref["nm"], gap, abs(h / ref["h_leaf"] - 1), abs(s - ref["slam_uncertainty"]) / s_tol, abs(w1 / ref["w1"] - 1),
        abs(w2 / ref["w2"] - 1), abs(out["unc"][i] / ref["uncertainty"] - 1), abs(out["cost"][i] / ref["cost"] - 1)))
    assert np.isnan(got[L:]).all(), name  # slots beyond the environment's landmarks are not written
    np.testing.assert_allclose(got[:L], want, rtol=K.LM_RTOL, atol=K.LM_ATOL, err_msg=name)
    assert h == pytest.approx(ref["h_leaf"], rel=sum_rtol), name
    assert abs(s - ref["slam_uncertainty"]) <= s_tol, name
    assert out["unc"][i] == w2 * h + w1 * s, name
    unc_tol = sum_rtol * 2 * abs(ref["w2"] * ref["h_leaf"]) + abs(ref["w1"]) * s_tol + abs(ref["w1"] * ref["slam_uncertainty"]) * root_rel
    assert abs(out["unc"][i] - ref["uncertainty"]) <= unc_tol, name
    dterm = ref["cost"] - ref["uncertainty"]
    assert abs(out["cost"][i] - ref["cost"]) <= unc_tol + 4e-16 * abs(dterm) + 2e-16 * abs(ref["cost"]), name


def live_state(eng, n_envs):
    """The bits of what the getters return of every environment's belief and map."""
    out = []
    for e in range(n_envs):
        out += [eng.poses(e)[0], eng.poses(e)[1], eng.landmarks(e)[1], eng.landmarks(e)[2], eng.virtual_map(e)[0], eng.virtual_map(e)[1]]
    return [bits(np.asarray(a, dtype=np.float64)) for a in out]


def check_nothing_else_moved(ctx, names, cases, between, fm2_names, em_name, delta_bound=None):
    """drlgx_fm2_update_steps / drlgx_em_cost_steps on the candidates `cases` (named `names`, handed over with a core mask) before
    and after the drlgx_slam_og_cost calls that `between` makes (a list of callables, one made before each), and the live belief
    and map through the getters: the getters return the same bits before and after.

    fm2_update and em_cost sum their prior with the fp64 atomics of k_fm2_prior, so two of THEIR calls need not give the same bits
    whatever runs between them (tests/test_gpu_fm2.py::test_mixed_launches).  As there: when three calls before the slam_og_cost
    call are bit-equal, the call after it must have those bits too; when they are not (observed on the MI355X, on the corridor's
    1333 factors and on the small world alike: a few ulp on a block's diagonal, more on its small off-diagonal elements), the
    call after it is held to the restatements exactly as the tests of those entries hold any call: the blocks of `fm2_names` (plans
    of ctx.world without a mask) to oracle/fm2_ref.py at rtol 1e-6 / atol 1e-10 and, where `delta_bound` gives the case one, the
    update term to it (tests/test_gpu_fm2.py); em_cost of `em_name`, both algorithms, through test_gpu_em._check_against_ref."""
    import fm2_cases as F
    from test_gpu_em import _check_against_ref
    from test_gpu_fm2 import _EmRef
    eng = ctx.eng
    ce, acts, nact, core = ctx.candidates(cases, masked=True)
    live0 = live_state(eng, len(ctx.sims))
    cov0, n0 = eng.fm2_update(ce, acts, nact, core=core)
    cov0b, _ = eng.fm2_update(ce, acts, nact, core=core)
    em0, em0b = eng.em_cost(ce, acts, nact, 1, core=core), eng.em_cost(ce, acts, nact, 1, core=core)
    cov0c, _ = eng.fm2_update(ce, acts, nact, core=core)   # (behind another entry's kernels, as the call after `between` is)
    em0c = eng.em_cost(ce, acts, nact, 1, core=core)
    between[0]()
    cov1, n1 = eng.fm2_update(ce, acts, nact, core=core)
    between[1]()
    em1 = eng.em_cost(ce, acts, nact, 1, core=core)
    assert eng.status() == 0
    for a, b in zip(live0, live_state(eng, len(ctx.sims))):
        np.testing.assert_array_equal(a, b)
    n0, n1 = n0.cpu().numpy(), n1.cpu().numpy()
    np.testing.assert_array_equal(n0, n1)
    cov0, cov0b, cov0c, cov1 = cov0.cpu().numpy(), cov0b.cpu().numpy(), cov0c.cpu().numpy(), cov1.cpu().numpy()
    fm2_stable = all(np.array_equal(bits(cov0[c, :n0[c]]), bits(other[c, :n0[c]])) for c in range(len(cases)) for other in (cov0b, cov0c))
    em_stable = all(np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())) for other in (em0b, em0c) for a, b in zip(em0, other))
    print("three calls before the slam_og_cost call bit-equal: fm2_update %s, em_cost %s" % (fm2_stable, em_stable))
    if fm2_stable:
        for c in range(len(cases)):
            np.testing.assert_array_equal(bits(cov0[c, :n0[c]]), bits(cov1[c, :n1[c]]))
    else:
        for name in fm2_names:
            ref, c = ctx.world.ref(name), names.index(name)
            assert cases[c][2] is None and n1[c] == ref["P"] + ref["K"], name
            got = cov1[c, :n1[c]]
            np.testing.assert_allclose(got, ref["cov"], rtol=F.SIGMA_RTOL, atol=F.SIGMA_ATOL, err_msg=name)
            if ref["nm"] and delta_bound is not None:
                ratio = np.abs((got - ref["base"]) - ref["delta"]).max() / np.abs(ref["delta"]).max()
                print("%s after the call: update term %.3e of max |Delta| (bound %.1e)" % (name, ratio, delta_bound[name]))
                assert ratio <= delta_bound[name], name
    if em_stable:
        for a, b in zip(em0, em1):
            np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    else:
        e, c = ctx.world.plans[em_name][0], names.index(em_name)
        assert cases[c][2] is None
        unc0, cost0, info = eng.em_cost(ce[c:c + 1].contiguous(), acts[c:c + 1].contiguous(), nact[c:c + 1].contiguous(), 0, want_info=True)
        emref = _EmRef(ctx)
        assert min(emref.ref(e, em_name)[3].values()) > 1e-9
        _check_against_ref(emref, e, em_name, float(unc0[0]), float(cost0[0]), float(em1[0][c]), float(em1[1][c]), info[0].cpu().numpy(),
                           "%s after the call" % em_name)
