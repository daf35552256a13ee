"""CPU tests of the restatements in tests/em_dubins_leaf_ref.py and of the cases in tests/em_dubins_leaf_cases.py, on the CPU
oracle's beliefs: the masked Woodbury form against an independent information-form solve, and every precondition that
tests/test_gpu_em_dubins_leaf.py relies on (and asserts again on the engine's own beliefs) - sensor-gate margins of the predicted
measurements, the masked and unmasked measurement counts, nearest-node and library-match margins of the trees."""
import numpy as np
import pytest

import em_dubins_cases as DC
import em_dubins_leaf_cases as LC
import em_dubins_leaf_ref as LR
import em_tree_cases as K
import em_tree_ref as R
import fm2_cases as F
from oracle import fm2_ref


@pytest.fixture(scope="module")
def world():
    return LC.steps_world()


@pytest.fixture(scope="module")
def refs(world):
    return {name: LR.fm2_update(world.sims[e], plan, core) for name, (e, plan, core) in LC.STEP_CASES.items()}


def test_all_core_is_the_unmasked_restatement(world):
    for name in ("one_edge", "ring33"):
        e, plan, _ = LC.STEP_CASES[name]
        got, n_meas = LR.fm2_update(world.sims[e], plan, [1] * len(plan))
        want, want_n = fm2_ref.fm2_update(world.sims[e], plan)
        assert got.tobytes() == want.tobytes() and n_meas == want_n, name


def test_masked_woodbury_form_agrees_with_the_information_form(world, refs):
    """The tolerance of the unmasked comparison of the two forms (tests/test_fm2_cpu.py): 1e-2 of the GPU test's."""
    for name, (e, plan, core) in LC.STEP_CASES.items():
        alt = LR.information_form(world.sims[e], plan, core)
        np.testing.assert_allclose(alt, refs[name][0], rtol=F.SIGMA_RTOL * 1e-2, atol=F.SIGMA_ATOL * 1e-2, err_msg=name)


def test_cases_are_what_they_claim(world, refs):
    for name, (e, plan, core) in LC.STEP_CASES.items():
        masked, total, margin = LR.masked_counts(world.sims[e], plan, core)
        assert masked == LC.NM[name] == sum(refs[name][1]) and masked <= F.MAX_MEAS, name
        assert margin > 1e-6, "%s sits on a knife edge (%.3e)" % (name, margin)
        assert len(plan) <= LC.MAX_ACTIONS and len(core) == len(plan)
    e, plan, core = LC.STEP_CASES["K_max"]
    assert len(plan) == LC.MAX_ACTIONS and LR.masked_counts(world.sims[e], plan, core)[1] > F.MAX_MEAS
    e, plan, core = LC.OVER
    masked, _, margin = LR.masked_counts(world.sims[e], plan, core)
    assert masked > F.MAX_MEAS and margin > 1e-6


def test_ignoring_the_mask_would_show(world, refs):
    """Every case with a non-core step inside the ring: the unmasked covariances lie many tolerances from the masked ones, and the
    unmasked cost far from the masked cost."""
    for name in ("one_edge", "two_edges", "trailing", "fresh_edge", "ring33"):
        e, plan, core = LC.STEP_CASES[name]
        plain, _ = fm2_ref.fm2_update(world.sims[e], plan)
        gap = np.abs(plain - refs[name][0]) / (F.SIGMA_RTOL * np.abs(refs[name][0]) + F.SIGMA_ATOL)
        assert gap.max() > 1e3, (name, gap.max())
    # the cost: steps 5 cm apart sweep the same cells, so it is the case whose non-core step alone enters the ring that shows it
    # (measured: 3.3e-3 relative for both algorithms, five cells that only the non-core step reaches)
    e, plan, core = LC.STEP_CASES["blind_core"]
    u_m, c_m, info_m, upd_m = LR.em_cost(world.sims[e], plan, core)
    u_p, c_p, info_p, upd_p = LR.em_cost(world.sims[e], plan, [1] * len(plan))
    assert abs(u_m - u_p) > 1e-3 * abs(u_p), (u_m, u_p)
    assert int((upd_p & ~upd_m).sum()) >= 1
    # a distance that is not the plan's own moves the cost by exactly its share
    _, c_d, _, _ = LR.em_cost(world.sims[e], plan, core, distance=LC.TREE_DISTANCE)
    assert c_d != c_m


@pytest.fixture(scope="module")
def sims():
    return DC.make_sims()


@pytest.mark.parametrize("name, sd", LC.TREE_CASES)
def test_tree_cases_have_their_margins(sims, name, sd):
    cfg = sims[0].cfg
    results, leaves = [], 0
    for e, s in enumerate(sims):
        keys, xy, _ = s.landmarks()
        t = LC.tree_of(cfg, s.poses()[0][-1], s.virtual_map()[0].reshape(-1), DC.library(name), DC.START_INDICES[e], keys, xy, sd)
        assert DC.entitled(t) and not t.full, (name, sd, e)
        cands = LR.leaf_candidates(t, DC.MAX_ACTIONS)
        results.append(t.result)
        leaves += len(cands)
        for node, rows, core, dist in cands:
            assert len(rows) == t.depth[node] <= DC.MAX_ACTIONS and int(core.sum()) >= 1 and core[len(rows) - 1] == 1
            masked, _, margin = LR.masked_counts(s, [tuple(r) for r in rows], core)
            assert masked <= F.MAX_MEAS and margin > 1e-9, (name, sd, e, node)
        if t.result == R.SUCCESS:
            assert len(cands) >= 2 and max(t.depth) > 5   # (the engine of 5 actions refuses such a tree)
    assert results.count(R.SUCCESS) >= 2 and leaves >= 6
    if (name, sd) in (("36", 0.0), ("320", DC.SAFE_DISTANCE)):
        assert R.SAMPLING_FAILURE in results


def test_a_tree_of_no_accepted_node_offers_its_root(sims):
    s, cfg = sims[0], sims[0].cfg
    t = LC.tree_of(cfg, s.poses()[0][-1], s.virtual_map()[0].reshape(-1), DC.library("36"), 0, (), (), 0.0, max_nodes=0.0)
    (node, rows, core, dist), = LR.leaf_candidates(t, DC.MAX_ACTIONS)
    assert node == 0 and len(rows) == 0 and core.sum() == 0 and dist == 0.0 and t.halton_next == 0
