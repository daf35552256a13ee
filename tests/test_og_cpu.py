"""The yardstick of the expected map entropy (tests/og_ref.py) checked on the CPU before tests/test_gpu_og.py uses it: against the
oracle's own virtual map where the two must agree (no action), against a case worked out by hand, and for the margins by which
the parity cases take their decisions.  No GPU."""
import math

import numpy as np
import pytest

import og_cases
import og_ref

# The geometric gates (range, field of view, the floors behind the cell indices) move with the poses, which device and oracle
# agree on to 1e-9 (1e-9 abs; a ray end point moves by the pose error plus max_range x the heading error).
# The cases keep 100 x that distance from every one of them.  The `> OCCUPIED_THRESH + 1e-8` branch does not depend on any pose:
# both sides are values of the ladder, the same sums of the same constants everywhere, and a cell that was never updated compares
# 0 against 1e-8 - a margin of exactly 1e-8 whatever the case.  It is asserted at the pose tolerance itself.
GEOMETRY_MARGIN = 1e-7
THRESH_MARGIN = 1e-9


@pytest.fixture(scope="module")
def sims():
    return {name: og_cases.make_sims(name) for name in og_cases.CONFIGS}


def test_zero_actions_reproduce_the_oracles_probabilities(sims):
    """Both are the same ladder from the same poses: exact."""
    for name, ss in sims.items():
        for e, sim in enumerate(ss):
            h, cost, prob, _ = og_ref.og_cost(sim, [])
            np.testing.assert_array_equal(prob, sim.virtual_map()[0], err_msg="%s env %d" % (name, e))
            assert cost == h  # no action, no distance
            assert len(np.unique(prob)) > 2, "the belief of %s env %d saw nothing" % (name, e)


def test_grids_are_the_shapes_the_gpu_tests_need(sims):
    assert sims["small"][0].vm_shape() == (6, 6) and sims["mid"][0].vm_shape() == (20, 20) and sims["sector"][0].vm_shape() == (6, 6)
    assert sum(og_cases.landmarks_outside_the_grid(s) for s in sims["small"]) > 0
    for name, ss in sims.items():
        for sim in ss:
            plans = og_cases.plans_for(sim)
            P = sim.num_poses()
            assert [len(p) for p in plans[:3]] == [0, 1, og_cases.MAX_ACTIONS]
            assert [P + len(p) for p in plans[3:6]] == [63, 64, 65]
            assert og_cases.leaves_the_map(sim, plans[6]) and len(plans[6]) <= og_cases.MAX_ACTIONS


def test_one_pose_one_landmark_by_hand():
    """The 6 x 6 grid of the "small" map (cell centres at -5, -3, ..., 5), one pose at (1.4, 0.6) heading along +x, one landmark
    at (3.2, 1.1).  Squared offsets of the centres from the pose: in x 40.96, 19.36, 5.76, 0.16, 2.56, 12.96, in y 31.36, 12.96,
    2.56, 0.16, 5.76, 19.36; the centres within 6 m (sum < 36) are 0 + 4 + 5 + 6 + 6 + 5 = 26 cells, column by column, and none
    of them is within 5 degrees of the blind ray behind the sensor.  The landmark's cell - centre (3, 1), row 3, column 4 - goes
    0 -> min(MAX, 0 + occupied) = MAX_LOGODDS = LOGODDS2PROB(0.95) = 0.72112 before the pose and, being above the threshold,
    gets `occupied` again: it stays there, p = 0.67285.  The other 25 seen cells get `free` once: p = 0.3.  The 10 unseen cells
    stay at p = 0.5."""
    cfg = og_cases.oracle_config("small")
    pose = np.array([[1.4, 0.6, 1.0, 0.0]])
    lo, margins = og_ref.occupancy_logodds(pose, np.array([[3.2, 1.1]]), cfg, 6, 6)
    lo = lo.reshape(6, 6)
    seen_per_col = [0, 4, 5, 6, 6, 5]
    for col in range(6):
        assert int(np.sum(lo[:, col] != 0.0)) == seen_per_col[col], col
    p_max = math.exp(0.95) / (1 + math.exp(0.95))
    assert lo[3, 4] == p_max and p_max == pytest.approx(0.72112, abs=1e-5)
    free = lo == math.log(0.3 / 0.7)
    assert int(free.sum()) == 25 and int((lo == 0.0).sum()) == 10
    prob = og_ref.probabilities(lo.reshape(-1), 1).reshape(6, 6)
    assert prob[3, 4] == pytest.approx(0.67285, abs=1e-5) and prob[free] == pytest.approx(0.3, abs=1e-15)
    h2 = lambda p: -p * math.log(p) - (1 - p) * math.log(1 - p)  # noqa: E731
    assert og_ref.entropy(prob.reshape(-1)) == pytest.approx(25 * h2(0.3) + h2(prob[3, 4]) + 10 * math.log(2), rel=1e-14)
    assert margins["thresh"] == 1e-8  # the untouched cells: 0 against 0 + 1e-8
    # a landmark outside the grid is ignored; a second pose leaves the clamped and the once-freed cells where the ladder says
    lo2, _ = og_ref.occupancy_logodds(pose, np.array([[3.2, 1.1], [7.5, 0.3]]), cfg, 6, 6)
    np.testing.assert_array_equal(lo2, lo.reshape(-1))
    lo3, _ = og_ref.occupancy_logodds(np.repeat(pose, 5, axis=0), np.array([[3.2, 1.1]]), cfg, 6, 6)
    lo3 = lo3.reshape(6, 6)
    assert lo3[3, 4] == p_max and np.all(lo3[free] == math.log(0.05 / 0.95)) and int((lo3 == 0.0).sum()) == 10


def test_no_parity_case_sits_on_a_knife_edge(sims):
    worst = {"range": math.inf, "bearing": math.inf, "floor": math.inf, "thresh": math.inf}
    for name, ss in sims.items():
        for sim in ss:
            for plan in og_cases.plans_for(sim):
                margins = og_ref.og_cost(sim, plan)[3]
                for k in worst:
                    worst[k] = min(worst[k], margins[k])
    print("smallest margins: " + ", ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    assert min(worst["range"], worst["bearing"], worst["floor"]) > GEOMETRY_MARGIN
    assert worst["thresh"] > THRESH_MARGIN
