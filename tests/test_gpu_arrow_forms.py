"""GPU: a full solve of the pose-chain solver (csrc/k_slam_arrow.hip) in every cell of its run-time choices - the worlds of
tests/arrow_cases.py, which tests/test_arrow_cases_cpu.py proves to be in their cells - against the CPU oracle.  Per case:

  (a) DRLGX_INCREMENTAL=0: every update is a full solve (mk_panel off) at the instance's counts; the state after the check
      step against the oracle's by compare_state of tests/test_gpu_belief.py, its tolerances unchanged, mask_knife_edge on.
  (b) the incremental update on: the check step relinearises, so it is a full solve that leaves the covariance panel (the
      full-solve counter of inc_stats advances by one per environment, the rank-k counter does not).  The panel - Sigma's
      columns of the newest pose and of every landmark - against the same columns of the oracle's full covariance: rtol 1e-7,
      the project's covariance-block tolerance, plus atol 1e-7 x the largest diagonal entry.  Then EXTRA_STEPS steps served
      by the rank-k update from that panel (the rank-k counter advances by one per environment and step), and compare_state.
      At 496 landmarks the rank-k update has no room in LDS (Case.rank_k_after): there the steps are asserted to be full solves.
  (c) poses, landmarks and factors of the engine equal the oracle's at the check step: the solve ran in the cell the CPU
      test proved.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import arrow_cases as A  # noqa: E402
from test_gpu_belief import compare_state  # noqa: E402


def _engine(case):
    from drl_graph_exploration_amd.engine import Engine
    eng = Engine(case.engine_config(), case.n, 0)
    eng.set_fixed_landmarks(case.fixed)
    eng.reset(np.arange(case.n), np.arange(case.n), starts=case.starts)
    return eng


def _step(eng, case, s):
    eng.step(torch.tensor(np.array([case.action(s)] * case.n, dtype=np.float64), device=eng.device))


def _counts_equal(eng, sims, what):
    for i, sim in enumerate(sims):
        c = eng.counts(i)
        assert (c["poses"], c["landmarks"], c["factors"]) == A.counts(sim), (what, i, c, A.counts(sim))


def _panel_against_oracle(eng, i, sim, what):
    """The panel's rows are the poses (3 each) then the landmarks by slot (2 each); its columns the newest pose (3) then the
    landmarks.  The oracle's full covariance is ordered landmarks by slot, then poses."""
    Sig, L, P = sim.full_covariance()
    meta, body = eng.panel(i)
    assert meta.tolist() == [1, P, L, len(sim.factors()[0])], (what, meta)
    rows = np.concatenate([2 * L + np.arange(3 * P), np.arange(2 * L)])
    cols = np.concatenate([2 * L + 3 * (P - 1) + np.arange(3), np.arange(2 * L)])
    want = Sig[np.ix_(rows, cols)]
    atol = 1e-7 * float(np.diag(Sig).max())
    print("%s env %d: panel %s, largest |panel - oracle| %.3e (largest diagonal entry %.3e), largest share of the tolerance %.3e" % (
        what, i, body.shape, np.abs(body - want).max(), np.diag(Sig).max(), (np.abs(body - want) / (atol + 1e-7 * np.abs(want))).max()))
    np.testing.assert_allclose(body, want, rtol=1e-7, atol=atol, err_msg=what)


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_full_solve_in_every_cell(case, monkeypatch):
    run = A.run_oracle(case)
    # (a) every update a full solve
    monkeypatch.setenv("DRLGX_INCREMENTAL", "0")
    eng = _engine(case)
    try:
        assert eng.inc_stats() == (-1, -1)
        for s in range(case.check_step + 1):
            _step(eng, case, s)
        assert eng.status() == 0
        _counts_equal(eng, run["check"], case.name + " (a)")                                           # (c)
        for i, sim in enumerate(run["check"]):
            compare_state(eng, i, sim, "%s (a) env %d" % (case.name, i), mask_knife_edge=True)
    finally:
        eng.close()
    # (b) the panel a full solve leaves, and the rank-k updates that consume it
    monkeypatch.delenv("DRLGX_INCREMENTAL")
    eng = _engine(case)
    try:
        for s in range(case.check_step):
            _step(eng, case, s)
        before = eng.inc_stats()
        _step(eng, case, case.check_step)
        at = eng.inc_stats()
        assert eng.status() == 0
        assert (at[0] - before[0], at[1] - before[1]) == (0, case.n), (before, at)
        _counts_equal(eng, run["check"], case.name + " (b)")                                           # (c)
        for i, sim in enumerate(run["check"]):
            _panel_against_oracle(eng, i, sim, case.name)
        for s in range(case.check_step + 1, case.n_steps):
            _step(eng, case, s)
        end = eng.inc_stats()
        assert eng.status() == 0
        served = A.EXTRA_STEPS * case.n
        assert (end[0] - at[0], end[1] - at[1]) == ((served, 0) if case.rank_k_after else (0, served)), (at, end)
        _counts_equal(eng, run["end"], case.name + " (b) end")
        for i, sim in enumerate(run["end"]):
            compare_state(eng, i, sim, "%s (b) env %d, %d updates behind the panel" % (case.name, i, A.EXTRA_STEPS), mask_knife_edge=True)
    finally:
        eng.close()
