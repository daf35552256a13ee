"""What tests/test_gpu_slam_og.py requires of the cases of tests/slam_og_cases.py and of the restatement tests/slam_og_ref.py,
checked on the CPU before anything runs on the device.  No GPU.

  * every case predicts the number of measurements it is named for and stays under the 256-measurement cap - all but the one case
    built to exceed it; no predicted pair sits within 1e-6 of a gate;
  * the restatement's information-form landmark blocks equal a covariance-form downdate (numpy as well) to 1e-10 relative;
  * closed forms: a plan that sees nothing leaves slam_uncertainty at the root's, so w1 * slam_uncertainty = alpha; alpha = 0 reduces
    the uncertainty to w2 * H_leaf; alpha = 1 drops the entropy; an environment without a landmark has w1 = inf;
  * the ini round-trip of `alpha`.
"""
import math

import numpy as np
import pytest

import fm2_cases as F
import og_ref
import slam_og_cases as K
import slam_og_ref as R


@pytest.fixture(scope="module")
def world():
    return K.world()


def test_cases_are_what_they_are_named_for(world):
    assert [s.num_poses() for s in world.sims] == [1, 4, 1]
    assert [s.num_landmarks() for s in world.sims] == K.RING_SIZES + [0]
    assert K.RING_SIZES[0] > 64 and K.CAPS["max_poses"] <= 24 and K.MAP == 20
    for name, (e, plan, core, nm) in list(K.CASES.items()) + [("overflow", K.OVERFLOW)]:
        ref_nm = sum(R._plan_rows(world.sims[e], plan, core)[2])
        assert ref_nm == nm, name
        assert (nm <= K.MAX_MEAS) == (name != "overflow"), name
        assert len(plan) <= K.CAPS["max_actions"]
        _, margin = F.predicted_pairs(world.sims[e], plan)
        assert margin > 1e-6, (name, margin)
    assert len(K.CASES["walked_K9"][1]) == K.CAPS["max_actions"] and len(K.CASES["walked_K1"][1]) == 1
    # without a mask the masked plan would predict twice as much: the mask is not inert
    e, plan, core, nm = K.CASES["walked_core"]
    assert sum(R._plan_rows(world.sims[e], plan, None)[2]) == 2 * nm


@pytest.mark.parametrize("case", sorted(K.CASES))
def test_information_form_equals_the_covariance_form_downdate(world, case):
    e, plan, core, nm = K.CASES[case]
    a, _ = R.landmark_blocks(world.sims[e], plan, core)
    b = R.landmark_blocks_downdate(world.sims[e], plan, core)
    gap = np.abs(a - b).max() / np.abs(a).max()
    print("%s: nm %d  information form against downdate %.2e of max |block|" % (case, nm, gap))
    assert gap <= 1e-10
    # ... and the update term is not lost in that: it moves the blocks by far more than the GPU test's tolerance
    if nm:
        prior = R.prior_landmark_blocks(world.sims[e])
        assert np.abs(a - prior).max() > 100 * (K.LM_RTOL * np.abs(a).max() + K.LM_ATOL)


def test_a_plan_that_sees_nothing_keeps_the_roots_term(world):
    for case in ("walked_blind", "walked_K0", "big_K0"):
        ref = K.reference(world, case)
        assert ref["nm"] == 0
        assert ref["w1"] * ref["slam_uncertainty"] == pytest.approx(K.ALPHA, rel=1e-9), case
        prior = R.prior_landmark_blocks(world.sims[K.CASES[case][0]])
        assert np.abs(ref["lm_cov"] - prior).max() <= 1e-10 * np.abs(prior).max()  # (another matrix is inverted: not the same bits)


def test_alpha_0_and_1(world):
    for case in ("big_K2", "walked_core"):
        e, plan, core, _ = K.CASES[case]
        h = og_ref.og_cost(world.sims[e], plan)[0]
        r0, r1 = K.reference(world, case, alpha=0.0), K.reference(world, case, alpha=1.0)
        assert r0["w1"] == 0.0 and r0["uncertainty"] == r0["w2"] * h
        assert r1["w2"] == 0.0 and r1["uncertainty"] == r1["w1"] * r1["slam_uncertainty"] and 0 < r1["uncertainty"] < 1
        # the sightings only ever remove landmark uncertainty: below the root's alpha = 1
        assert r0["cost"] - r0["uncertainty"] == pytest.approx(r1["cost"] - r1["uncertainty"], rel=1e-12)


def test_no_landmark_gives_an_infinite_weight(world):
    w1, w2 = R.root_weights(world.sims[K.BLIND_ENV], K.ALPHA)
    assert w1 == math.inf and 0 < w2 < math.inf
    ref = R.slam_og_cost(world.sims[K.BLIND_ENV], [K.SHORT], K.ALPHA)
    assert ref["slam_uncertainty"] == 0.0 and math.isnan(ref["uncertainty"])  # inf * 0, as IEEE gives it


def test_caller_distance_replaces_the_plans_own(world):
    ref, far = K.reference(world, "walked_K1"), K.reference(world, "walked_K1", distance=7.25)
    assert far["uncertainty"] == ref["uncertainty"]
    assert far["cost"] - far["uncertainty"] == pytest.approx(7.25 * R.distance_weight(world.sims[1]), rel=1e-15)


def _ini(**planner):
    from configparser import ConfigParser
    cp = ConfigParser()
    cp.read_dict({
        "Sensor Model": dict(bearing_noise="0.5", range_noise="0.02", min_bearing="-179.9", max_bearing="179.9", min_range="0.1", max_range="6.0"),
        "Control Model": dict(translation_noise="0.1", rotation_noise="0.2"),
        "Environment": dict(min_x="-10", max_x="10", min_y="-10", max_y="10", max_steps="5000", safe_distance="0.0"),
        "Virtual Map": dict(resolution="2.0", sigma0="1.0", num_samples="1"),
        "Simulator": dict(seed="3", lo="3", num="8", sigma_x0="0.05", sigma_y0="0.05", sigma_theta0="0.01"),
        "Planner": dict(dict(seed="3", angle_weight="0.4", distance_weight0="5.0", distance_weight1="2.0", d_weight="0.0", max_edge_length="2.0",
                             max_nodes="0.5", occupancy_threshold="0.4", safe_distance="1.0", algorithm="EM_AOPT", reg_out="false"), **planner),
    })
    return cp


def test_alpha_ini_round_trip(tmp_path):
    """`alpha` of the [Planner] section reaches EMPlannerParameter through a written and re-read ini file; without the key the
    parameter keeps its default."""
    from drl_graph_exploration_amd import planner2d, pyplanner2d
    assert planner2d.EMPlannerParameter().alpha == 0.5
    assert pyplanner2d.config_from_ini(_ini())[1]["planner"].alpha == 0.5
    out = tmp_path / "slam_og.ini"
    with open(out, "w") as f:
        _ini(algorithm="SLAM_OG_SHANNON", alpha="0.125").write(f)
    cfg, prm = pyplanner2d.config_from_ini(pyplanner2d.load_config(str(out)))
    assert prm["planner"].alpha == 0.125 and prm["planner"].algorithm == planner2d.OptimizationAlgorithm.SLAM_OG_SHANNON
    assert cfg.algorithm == 3  # (what drlgx_create is handed is unchanged)
