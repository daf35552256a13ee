"""The yardstick of the expected look-ahead cost (tests/em_ref.py) checked on the CPU before tests/test_gpu_em.py uses it:
against the oracle's own virtual map where the two must agree (no action), against a case worked out by hand, and for the
properties the leaf evaluation has by construction.  No GPU."""
import math

import numpy as np
import pytest

import em_cases
import em_ref
from oracle import fm2_ref
from oracle import oracle as O

# Measured on the CPU (4 environments of em_cases.make_sims): with no action the restatement is at most 3.8e-12 (relative, entries
# above 1e-9; 7.1e-12 absolute on the off-diagonal entries near zero) away from the oracle's cell information, and 2.2e-16 /
# 1.1e-16 away from its A-opt / D-opt uncertainty - round-off of two fp64 inversions of the same matrices.  Asserted at 10x.
ZERO_ACTION_INFO_RTOL, ZERO_ACTION_INFO_ATOL, ZERO_ACTION_UNC_RTOL = 4e-11, 7.1e-11, 2.2e-15


@pytest.fixture(scope="module")
def sims():
    return em_cases.make_sims()[0]


def _oracle_info(sim):
    ov = sim.virtual_map()[1]
    return np.stack([ov[:, 0, 0], ov[:, 0, 1], ov[:, 1, 1]], axis=1)


def test_zero_actions_reproduce_the_oracles_virtual_map(sims):
    for e, sim in enumerate(sims):
        unc, cost, info, margins = em_ref.em_cost(sim, [], 0)
        want = _oracle_info(sim)
        gap = np.abs(info - want)
        print("env %d: info gap rel %.3e abs %.3e" % (e, np.max(gap[np.abs(want) > 1e-9] / np.abs(want[np.abs(want) > 1e-9])), gap.max()))
        np.testing.assert_allclose(info, want, rtol=ZERO_ACTION_INFO_RTOL, atol=ZERO_ACTION_INFO_ATOL, err_msg="env %d" % e)
        # topology: the same cells were never updated
        i0 = 1.0 / sim.cfg.sigma0 ** 2
        untouched = (info[:, 0] == i0) & (info[:, 1] == 0.0) & (info[:, 2] == i0)
        np.testing.assert_array_equal(untouched, sim.virtual_map()[3] == 0)
        assert unc == pytest.approx(sim.uncertainty_em(0), rel=ZERO_ACTION_UNC_RTOL)
        assert cost == unc  # no action, no distance
        assert em_ref.em_cost(sim, [], 1)[0] == pytest.approx(sim.uncertainty_em(1), rel=ZERO_ACTION_UNC_RTOL)


def test_one_pose_by_hand():
    """One pose at (1, 1) heading along +x with a diagonal information.  The cell centred at (3, 1) lies straight ahead at 2 m:
    d = (2, 0), so Hx = [[0, -1/2, -1], [-1, 0, 0]], Hl = [[0, 1/2], [1, 0]] and, with Sigma = diag(sx, sy, st),
    S = R + Hx Sigma Hx^T = diag(sb^2 + sy / 4 + st, sr^2 + sx); the cell's information is Hl^T S^-1 Hl =
    diag(1 / (sr^2 + sx), 1 / (4 sb^2 + sy + 4 st)).  The cell centred at (-1, 1) lies on the blind ray behind the sensor
    (bearing pi > max_bearing): it keeps I / sigma0^2."""
    cfg = O.default_config(em_cases.MAP)
    rows = cols = int((cfg.map_max_x - cfg.map_min_x) / cfg.resolution)
    sx, sy, st = 0.04, 0.09, 0.0025
    pose = np.array([[1.0, 1.0, 1.0, 0.0]])
    info, upd, gate_margin, _ = em_ref.update_information(pose, np.array([np.diag([1 / sx, 1 / sy, 1 / st])]), cfg, rows, cols)
    cell = lambda x, y: int((y - cfg.map_min_y) // cfg.resolution) * cols + int((x - cfg.map_min_x) // cfg.resolution)  # noqa: E731
    ahead, behind = cell(3.0, 1.0), cell(-1.0, 1.0)
    Hx = np.array([[0.0, -0.5, -1.0], [-1.0, 0.0, 0.0]])
    Hl = np.array([[0.0, 0.5], [1.0, 0.0]])
    R = np.diag([cfg.bearing_noise ** 2, cfg.range_noise ** 2])
    want = Hl.T @ np.linalg.inv(R + Hx @ np.diag([sx, sy, st]) @ Hx.T) @ Hl
    np.testing.assert_allclose(want, np.diag([1 / (cfg.range_noise ** 2 + sx), 1 / (4 * cfg.bearing_noise ** 2 + sy + 4 * st)]), rtol=1e-13)
    assert upd[ahead]
    np.testing.assert_allclose(info[ahead], want, rtol=1e-12, atol=1e-12)
    assert not upd[behind]
    np.testing.assert_array_equal(info[behind], np.eye(2) / cfg.sigma0 ** 2)
    # a pose whose information is (numerically) singular updates nothing
    info2, upd2, _, _ = em_ref.update_information(pose, np.array([np.diag([1e-4, 1e-4, 1e-4])]), cfg, rows, cols)
    assert not upd2.any()


def test_covariance_intersection_identities():
    """for m1 = m2 every weight gives m1 - in exact arithmetic; the reference's formula is 0 / 0 there
    (a = b, c = 2a, d = 0), so the identity is checked in the limit m2 -> m1 and the finite cases against the oracle's own
    covarianceIntersection2D."""
    m = np.array([[2.0, 0.3], [0.3, 1.0]])
    for eps in (1e-3, 1e-5):
        out = em_ref.covariance_intersection_2d(m, m * (1 + eps))
        np.testing.assert_allclose(out, m, rtol=1.01 * eps)  # a convex combination of m and (1 + eps) m, or one of the two
    rng = np.random.RandomState(3)
    L, out = O.lib(), np.zeros(4)
    for _ in range(50):
        a, b = rng.uniform(-1, 1, (2, 2)), rng.uniform(-1, 1, (2, 2))
        m1, m2 = a @ a.T + 0.1 * np.eye(2), b @ b.T * rng.choice([1.0, 30.0]) + 0.1 * np.eye(2)
        L.orc_kat_ci(O._dp(np.ascontiguousarray(m1.reshape(4))), O._dp(np.ascontiguousarray(m2.reshape(4))), O._dp(out))
        np.testing.assert_allclose(em_ref.covariance_intersection_2d(m1, m2).reshape(4), out, rtol=1e-9, atol=1e-12)
    # the inverted clamp: m1 >> m2 gives w < 0 with d > 0 -> w = 1 -> m1
    np.testing.assert_array_equal(em_ref.covariance_intersection_2d(100 * np.eye(2), np.eye(2)), 100 * np.eye(2))


def test_an_action_without_sightings_never_lowers_information(sims):
    for e, sim in enumerate(sims):
        plan = em_cases.blind_jump(sim)
        cov, n_meas = fm2_ref.fm2_update(sim, plan)
        assert sum(n_meas) == 0
        P = sim.num_poses()
        root_info = sim.poses()[1]
        for i in range(P):  # information of an old pose: leaf - root is positive semi-definite (here: the same matrix)
            diff = np.linalg.inv(cov[i]) - root_info[i]
            assert np.linalg.eigvalsh((diff + diff.T) / 2).min() >= -1e-6 * np.abs(root_info[i]).max(), (e, i)
        # the new pose covers cells nobody has seen (p = 0.5 > 0.49, information I / sigma0^2): the A-opt uncertainty drops
        prob = sim.virtual_map()[0].reshape(-1)
        upd_root = sim.virtual_map()[3] != 0
        unc, _, info, _ = em_ref.em_cost(sim, plan, 0)
        i0 = 1.0 / sim.cfg.sigma0 ** 2
        newly = ~upd_root & ~((info[:, 0] == i0) & (info[:, 1] == 0.0) & (info[:, 2] == i0))
        assert (newly & (prob > 0.49)).sum() > 0
        assert unc <= sim.uncertainty_em(0)


def test_no_parity_case_sits_on_a_knife_edge(sims):
    """What tests/test_gpu_em.py requires of its cases, checked here first: every range / field-of-view gate, every det < 1e-10
    and every probability threshold is decided by more than 1e-9."""
    from drl_graph_exploration_amd import default_config
    A = default_config(em_cases.MAP, num_landmarks=em_cases.NUM_LANDMARKS, max_poses=64).max_actions
    worst = math.inf
    for sim in sims:
        for plan in em_cases.plans_for(sim, A):
            assert len(plan) <= A
            assert sum(fm2_ref.fm2_update(sim, plan)[1]) <= 256
            worst = min(worst, min(em_ref.em_cost(sim, plan, 0)[3].values()))
    print("smallest margin %.3e" % worst)
    assert worst > 1e-9
