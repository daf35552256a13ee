"""TEST INFRASTRUCTURE: numpy (fp64) restatement of `calculateUncertainty_SLAM_OG_SHANNON` (src/em_exploration/Planner2D.cpp:394-416),
`costFunction` (:418-420) and the root weights of `EMPlanner2D::initialize` (:1341-1354) for one action list on an
`oracle.OracleSim`, written from the mathematics:

  * `updateTrajectory_SLAM_OG_SHANNON` (:584-618) adds the plan's noise-free odometry factors and predicted bearing-range factors to
    a copy of the root's iSAM2 and reads every landmark's marginal covariance.  With zero residuals and no relinearisation that is
    linear, and it is evaluated here in INFORMATION form - the route the kernel does not take: the joint information matrix of the
    belief's factors at the linearisation point (fm2_cases.information_matrix), the plan's poses appended with their odometry rows,
    the predicted measurement rows added, one dense inverse, the landmarks' 2x2 diagonal blocks read off.  (k_fm2.hip works in
    covariance form: the dense prior, T = I + A Sigma A^T, cross covariances by F chains.)
  * Jacobians, gates and the predicted-pose chain are oracle/fm2_ref.py's.
  * slam_uncertainty = sum_l sqrt(det Sigma'(l, l)); H_leaf = og_ref's entropy of the same leaf;
    w2 = (1 - alpha) / H(live virtual map), w1 = alpha / sum_l sqrt(det(inverse(information_l))) of the live landmark marginals;
    uncertainty = w2 H_leaf + w1 slam_uncertainty; cost = uncertainty + distance * distance_weight with og_ref's distance terms.

`landmark_blocks_downdate` is the same update a third way, for tests/test_slam_og_cpu.py: covariance form in numpy.
"""
import math

import numpy as np

import em_ref
import fm2_cases
import og_ref
from oracle import fm2_ref


def _plan_rows(sim, plan, core=None):
    """The whitened Jacobian rows the plan adds, over the variables [landmarks by slot (2 each), P old poses, K new poses (3 each)]:
    (odometry rows [3K, n], measurement rows [2 nm, n], n_meas per action).  core (a sequence of K flags or None = all): only core
    poses predict measurements."""
    cfg = sim.cfg
    P, L, K = sim.num_poses(), sim.num_landmarks(), len(plan)
    thp, _, thl, _, _ = sim.isam_state()
    n = 2 * L + 3 * (P + K)
    px = lambda i: slice(2 * L + 3 * i, 2 * L + 3 * i + 3)   # noqa: E731
    sig = np.array([cfg.translation_noise, cfg.translation_noise, cfg.rotation_noise])
    sig_br = np.array([cfg.bearing_noise, cfg.range_noise])
    origin, val0 = fm2_ref._pose(*sim.poses()[0][-1]), fm2_ref._pose(*thp[-1])
    keys, est, _ = sim.landmarks()
    slot_of = {int(k): j for j, k in enumerate(sim.slot_keys())}
    est_slot = np.zeros((L, 2))
    for key, xy in zip(keys, est):
        est_slot[slot_of[int(key)]] = xy
    odo, meas, n_meas = [], [], []
    for k, a in enumerate(plan):
        odom = fm2_ref._pose(*a)
        end = fm2_ref._compose(origin, odom)
        hx, H1b = fm2_ref._between(val0, end)
        h, _ = fm2_ref._between(odom, hx)
        Hl = np.array([[h[2], h[3], 0], [-h[3], h[2], 0], [0, 0, 1.0]])
        J = np.zeros((3, n))
        J[:, px(P + k - 1)], J[:, px(P + k)] = (Hl @ H1b) / sig[:, None], Hl / sig[:, None]
        odo.append(J)
        cnt = 0
        if core is None or core[k]:
            for j in range(L):  # slot order, as fm2_ref.fm2_update takes them
                dx, dy = est_slot[j][0] - end[0], est_slot[j][1] - end[1]
                rng = math.sqrt(dx * dx + dy * dy)
                bearing = math.atan2(-end[3] * dx + end[2] * dy, end[2] * dx + end[3] * dy)
                if cfg.min_range < rng < cfg.max_range and cfg.min_bearing < bearing < cfg.max_bearing:
                    Jx, Jl = fm2_ref._br_jacobians(end, thl[j])
                    J = np.zeros((2, n))
                    J[:, px(P + k)], J[:, 2 * j:2 * j + 2] = Jx / sig_br[:, None], Jl / sig_br[:, None]
                    meas.append(J)
                    cnt += 1
        n_meas.append(cnt)
        origin, val0 = end, end
    return (np.concatenate(odo) if odo else np.zeros((0, n))), (np.concatenate(meas) if meas else np.zeros((0, n))), n_meas


def _blocks(Sig, L):
    return np.array([Sig[2 * j:2 * j + 2, 2 * j:2 * j + 2] for j in range(L)]).reshape(L, 2, 2)


def prior_landmark_blocks(sim):
    """The landmarks' 2x2 blocks of the inverse of the belief's information matrix, slot order."""
    return _blocks(np.linalg.inv(fm2_cases.information_matrix(sim)), sim.num_landmarks())


def landmark_blocks(sim, plan, core=None):
    """INFORMATION form.  Returns (blocks [L, 2, 2] in slot order, n_meas per action)."""
    P, L, K = sim.num_poses(), sim.num_landmarks(), len(plan)
    n0, n = 2 * L + 3 * P, 2 * L + 3 * (P + K)
    odo, meas, n_meas = _plan_rows(sim, plan, core)
    Lam = np.zeros((n, n))
    Lam[:n0, :n0] = fm2_cases.information_matrix(sim)
    Lam += odo.T @ odo + meas.T @ meas
    return _blocks(np.linalg.inv(Lam), L), n_meas


def landmark_blocks_downdate(sim, plan, core=None):
    """COVARIANCE form: Sigma (the belief and the plan's odometry, no sighting) downdated by the measurement rows A,
    Sigma' = Sigma - Sigma A^T (I + A Sigma A^T)^-1 A Sigma."""
    P, L, K = sim.num_poses(), sim.num_landmarks(), len(plan)
    n0, n = 2 * L + 3 * P, 2 * L + 3 * (P + K)
    odo, A, _ = _plan_rows(sim, plan, core)
    Lam = np.zeros((n, n))
    Lam[:n0, :n0] = fm2_cases.information_matrix(sim)
    Sig = np.linalg.inv(Lam + odo.T @ odo)
    if len(A):
        SA = Sig @ A.T
        Sig = Sig - SA @ np.linalg.solve(np.eye(len(A)) + A @ SA, SA.T)
    return _blocks(Sig, L)


def sum_sqrt_det(blocks):
    """sum_l sqrt(det), the landmarks in the order given (0 for none)."""
    s = 0.0
    for b in blocks:
        s += math.sqrt(b[0, 0] * b[1, 1] - b[0, 1] * b[1, 0])
    return s


def root_weights(sim, alpha):
    """(w1, w2) of EMPlanner2D::initialize from the live belief: the landmark marginals (slot order) and the live map."""
    keys, _, info = sim.landmarks()
    slot_of = {int(k): j for j, k in enumerate(sim.slot_keys())}
    cov = [None] * len(keys)
    for key, m in zip(keys, info):
        cov[slot_of[int(key)]] = np.linalg.inv(m)
    s = sum_sqrt_det(cov)
    h = og_ref.entropy(sim.virtual_map()[0].reshape(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(alpha) / np.float64(s)), float(np.float64(1.0 - alpha) / np.float64(h))


def slam_og_cost(sim, plan, alpha, core=None, distance=None):
    """dict(uncertainty, cost, h_leaf, slam_uncertainty, w1, w2, lm_cov [L, 2, 2] slot order, n_meas, nm) of the leaf that `plan`
    reaches from the belief of `sim`."""
    plan = [tuple(float(v) for v in a) for a in plan]
    blocks, n_meas = landmark_blocks(sim, plan, core)
    s = sum_sqrt_det(blocks)
    h_leaf = og_ref.og_cost(sim, plan)[0]
    w1, w2 = root_weights(sim, alpha)
    unc = w2 * h_leaf + w1 * s
    own = em_ref.plan_distance(plan, sim.cfg.angle_weight)
    dterm = (own if distance is None else distance) * distance_weight(sim)
    return dict(uncertainty=unc, cost=unc + dterm, h_leaf=h_leaf, slam_uncertainty=s, w1=w1, w2=w2, lm_cov=blocks, n_meas=n_meas,
                nm=int(sum(n_meas)))


def distance_weight(sim):
    """costFunction's distance weight from the LIVE map's probabilities (og_ref.og_cost's expression)."""
    cfg = sim.cfg
    rows, cols = sim.vm_shape()
    known = int(np.sum(sim.virtual_map()[0] < cfg.occupancy_threshold))
    return cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * (known / float(rows * cols))
