"""CPU checks, with the oracle and the host-only drlgx_debug_arrow_form alone, that the worlds of tests/arrow_cases.py put a full
solve of the pose-chain solver into the cell they claim - before tests/test_gpu_arrow_forms.py relies on them on the device:

  C1  at the check step both environments hold exactly P poses and all L landmarks, and their (P, L, M) - num_poses,
      num_landmarks, the number of bearing-range factors - are in the claimed cell by drlgx_debug_arrow_form with mk_panel 0
      and 1, and in every row of ROWS the case lists;
  C2  no listed landmark lies within 1e-6 (m, rad) of the range or field-of-view limits at any ground-truth pose: a 1-ulp
      difference of a measurement cannot change the topology;
  C3  the check step's update relinearises (with the incremental update on it is a full solve that leaves the panel) and no
      later step brings a first sighting or more than 64 factors (the steps behind it are rank-k updates);
  C4  the twelve rows of the case table are all claimed, and the host function rejects what the kernel does not serve.

Printed with -s: the counts, the margins and the oracle's time per case.
"""
import ctypes as C
import time

import pytest

import arrow_cases as A


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_case_is_in_its_cell(case):
    t0 = time.time()
    fresh = case.name not in A._runs
    run = A.run_oracle(case)
    dt = time.time() - t0
    forms = []
    for sim in run["check"]:
        P, L, M = A.counts(sim)
        assert (P, L) == (case.P, case.L), (P, L)                                                     # C1
        assert M >= L
        for mk in (0, 1):
            got = A.arrow_form(P, L, M, case.L_max, mk)
            assert case.matches(got), (case.name, (P, L, M), mk, got, case.cell)
            for row in case.rows:
                assert A.ROWS[row](got, L), (case.name, row, got)
        forms.append(((P, L, M), got))
    print("\n%s: %s  range margin %.3e m, field-of-view margin %.3e rad, largest later step + %d factors%s" % (
        case.name, forms, run["margin"][0], run["margin"][1], run["new_factors"], ", oracle %.1f s" % dt if fresh else ""))
    assert min(run["margin"]) > 1e-6                                                                  # C2
    assert all(run["relin"]), run["relin"]                                                            # C3
    assert run["new_landmarks"] == 0 and 0 < run["new_factors"] <= 64
    for sim in run["end"]:
        assert sim.num_poses() == case.P + A.EXTRA_STEPS and sim.num_landmarks() == case.L
        assert len(sim.factors()[0]) <= case.caps["max_factors"]


def test_every_row_of_the_case_table_is_claimed():
    claimed = {r for c in A.CASES for r in c.rows}
    assert claimed == set(A.ROWS), sorted(set(A.ROWS) - claimed)                                      # C4
    assert len({c.name for c in A.CASES}) == len(A.CASES) and all(c.n == 2 for c in A.CASES)
    # the rank-k update serves the steps behind the check step everywhere but at 496 landmarks (no room for its Y rows in LDS)
    assert [c.name for c in A.CASES if not c.rank_k_after] == ["stream496_obs_ws"]


def test_host_function_rejects_what_no_kernel_serves():
    """64 landmarks in an engine of max_landmarks 63 (k_slam_arrow<0> has no workspace sweep: ArrowCtx::setup leaves), counts
    out of range; and the vector form, which no case reaches beyond 53 poses, below 7 landmarks."""
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    out = (C.c_int32 * 9)()
    assert L.drlgx_debug_arrow_form(60, 64, 100, 63, 0, out) != 0
    assert L.drlgx_debug_arrow_form(0, 3, 10, 40, 0, out) != 0 and L.drlgx_debug_arrow_form(5, 41, 10, 40, 0, out) != 0
    assert L.drlgx_debug_arrow_form(5, 3, -1, 40, 0, out) != 0 and L.drlgx_debug_arrow_form(5, 3, 10, 40, 0, None) != 0
    assert A.arrow_form(60, 6, 100, 40, 1)["form"] == A.VECTOR and A.arrow_form(60, 7, 100, 40, 1)["form"] == A.TILES
    assert A.arrow_form(60, 64, 100, 64, 1)["form"] == A.TILES and A.arrow_form(60, 65, 100, 65, 1)["form"] == A.STAGED
    assert A.arrow_form(60, 63, 100, 63, 0)["system"] == A.PACKED and A.arrow_form(60, 63, 100, 64, 0)["system"] == A.PACKED
