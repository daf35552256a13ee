"""TEST INFRASTRUCTURE: numpy (fp64) restatement of the leaf evaluation of `EMPlanner2D::optimize2`
(src/em_exploration/Planner2D.cpp:1095-1104) for one action list on an `oracle.OracleSim`:

  * `updateTrajectory_EM` (:472-551): the covariances of `oracle.fm2_ref.fm2_update`; every pose is a core pose of the leaf's map
    with information = cov.inverse() (:521-523) - the old ones at the current estimate (`sim.poses()`), the new ones at the
    noise-free predicted poses, chained as fm2_ref chains them;
  * `VirtualMap::updateInformation(map)` (VirtualMap.cpp:256-316) on a copy of the root's virtual map: every cell back to
    I / sigma0^2, the poses in trajectory order, `predictVirtualLandmark` (:213-229) and `covarianceIntersection2D` (:364-378) in
    the REFERENCE's form (the pseudo-inverse of Hl and the two inversions, not the device's rearranged
    algebra); the probabilities stay those of `sim.virtual_map()`;
  * `calculateUncertainty_EM` (:321-341), `costFunction` (:418-420) with the distance weight of `initialize` (:1322-1332) and the
    distance of `simulations_reward` (:1440).

Besides the values it reports by how little any decision was taken: the smallest distance of a (pose, cell) pair from a range /
field-of-view gate, of a pose's det(information) from 1e-10, of a cell's probability from 0.49 / the occupancy threshold.
"""
import math

import numpy as np

from oracle import fm2_ref


def predict_virtual_landmark(pose, info, pt, cfg):
    """VirtualMap::predictVirtualLandmark: pose (x, y, cos, sin), info 3x3, pt (x, y).  Returns (2x2 information or None, the
    smallest margin of the gates that decided)."""
    dx, dy = pt[0] - pose[0], pt[1] - pose[1]
    rng = math.sqrt(dx * dx + dy * dy)
    margin = abs(rng - cfg.max_range)
    if not rng < cfg.max_range:                      # searchVirtualLandmarkNeighbors(state, max_range): dist < radius
        return None, margin
    qx, qy = pose[2] * dx + pose[3] * dy, -pose[3] * dx + pose[2] * dy
    bearing = math.atan2(qy, qx)
    margin = min(margin, abs(rng - cfg.min_range), abs(bearing - cfg.max_bearing), abs(bearing - cfg.min_bearing))
    if not (bearing < cfg.max_bearing and bearing > cfg.min_bearing and rng < cfg.max_range and rng > cfg.min_range):
        return None, margin                          # BearingRangeSensorModel::check
    Hx, Hl = fm2_ref._br_jacobians(pose, pt)         # rows: bearing, range (Pose2::bearing / Pose2::range)
    R = np.diag([cfg.bearing_noise, cfg.range_noise])
    R = R @ R
    Hp = np.linalg.inv(Hl.T @ Hl) @ Hl.T             # Hl = (Hl^T Hl)^-1 Hl^T
    cov = Hp @ (R + Hx @ np.linalg.solve(info, Hx.T)) @ Hp.T
    return np.linalg.inv(cov), margin


def covariance_intersection_2d(m1, m2):
    """VirtualMap::covarianceIntersection2D, with its two inverted clamps."""
    a = np.linalg.det(m1)
    b = np.linalg.det(m2)
    c = a * np.trace(np.linalg.solve(m1, m2))
    d = a + b - c
    w = 0.5 * (2 * b - c) / d
    if (w < 0 and d < 0) or (w > 1 and d > 0):
        w = 0.0
    elif (w < 0 and d > 0) or (w > 1 and d < 0):
        w = 1.0
    return w * m1 + (1.0 - w) * m2


def update_information(poses, infos, cfg, rows, cols):
    """VirtualMap::updateInformation(map): poses [n, 4], infos [n, 3, 3] in trajectory order, all core.  Returns
    (info [V, 2, 2], updated [V] bool, gate margin, det margin)."""
    V = rows * cols
    i0 = 1.0 / cfg.sigma0 ** 2
    out = np.tile(np.array([[i0, 0.0], [0.0, i0]]), (V, 1, 1))
    upd = np.zeros(V, dtype=bool)
    cx = (np.arange(cols) + 0.5) * cfg.resolution + cfg.map_min_x
    cy = (np.arange(rows) + 0.5) * cfg.resolution + cfg.map_min_y
    X, Y = np.meshgrid(cx, cy)
    X, Y = X.reshape(-1), Y.reshape(-1)
    gate_margin, det_margin = math.inf, math.inf
    for pose, info in zip(poses, infos):
        det = np.linalg.det(info)
        det_margin = min(det_margin, abs(det - 1e-10))
        if det < 1e-10:
            continue
        rng = np.sqrt((X - pose[0]) ** 2 + (Y - pose[1]) ** 2)
        gate_margin = min(gate_margin, float(np.min(np.abs(rng - cfg.max_range))))
        for v in np.nonzero(rng < cfg.max_range + 1e-6)[0]:  # (a superset of the radius query: predict decides)
            new, m = predict_virtual_landmark(pose, info, (X[v], Y[v]), cfg)
            gate_margin = min(gate_margin, m)
            if new is None:
                continue
            if upd[v]:
                out[v] = covariance_intersection_2d(out[v], new)
            else:
                out[v] = new
                upd[v] = True
    return out, upd, gate_margin, det_margin


def leaf_poses(sim, actions):
    """The leaf's trajectory as (x, y, cos, sin): the estimates, then the predicted poses chained as fm2_ref chains them."""
    xyt, _ = sim.poses()
    poses = [fm2_ref._pose(*p) for p in xyt]
    origin = poses[-1]
    for a in actions:
        origin = fm2_ref._compose(origin, fm2_ref._pose(*a))
        poses.append(origin)
    return np.array(poses)


def plan_distance(actions, angle_weight):
    """Planner2D.cpp:1440: dist += sqrt(x^2 + y^2 + angle_weight * theta^2), theta = Pose2::theta() (wrapped)."""
    dist = 0.0
    for x, y, th in actions:
        th = math.atan2(math.sin(th), math.cos(th))
        dist = dist + math.sqrt(x * x + y * y + angle_weight * (th * th))
    return dist


def uncertainty(info, prob, algorithm):
    """calculateUncertainty_EM: info [V, 2, 2], prob [V]."""
    w = (prob > 0.49).astype(np.float64)
    if algorithm == 1:
        return float(np.sum(w / np.linalg.det(info)))
    return float(np.sum(w * np.trace(np.linalg.inv(info), axis1=1, axis2=2)))


def em_costs(sim, actions, cov=None):
    """em_cost for both algorithms from one rebuild: ((uncertainty, cost) of EM_AOPT, (uncertainty, cost) of EM_DOPT, info, margins)."""
    u0, c0, info, margins = em_cost(sim, actions, 0, cov)
    prob = sim.virtual_map()[0].reshape(-1)
    u1 = float(np.sum((prob > 0.49) / (info[:, 0] * info[:, 2] - info[:, 1] * info[:, 1])))
    return (u0, c0), (u1, u1 + (c0 - u0)), info, margins


def em_cost(sim, actions, algorithm=0, cov=None):
    """(uncertainty, cost, info [V, 3] = xx xy yy, margins) of the leaf that `actions` reach from the belief of `sim`;
    margins = {"gate", "det", "prob"}: by how little the closest decision of each kind was taken.  cov: the pose covariances
    [P + K, 3, 3] instead of fm2_ref's (to measure the sensitivity to them)."""
    cfg = sim.cfg
    actions = [tuple(float(v) for v in a) for a in actions]
    if cov is None:
        cov, _ = fm2_ref.fm2_update(sim, actions)
    poses = leaf_poses(sim, actions)
    infos = np.array([np.linalg.inv(c) for c in cov])        # cov.inverse()
    rows, cols = sim.vm_shape()
    info, _, gate_margin, det_margin = update_information(poses, infos, cfg, rows, cols)
    prob = sim.virtual_map()[0].reshape(-1)                  # the leaf's virtual map is a copy of the root's
    unc = uncertainty(info, prob, algorithm)
    known = int(np.sum(prob < cfg.occupancy_threshold))
    dw = cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * (known / float(rows * cols))
    cost = unc + plan_distance(actions, cfg.angle_weight) * dw
    prob_margin = float(min(np.min(np.abs(prob - 0.49)), np.min(np.abs(prob - cfg.occupancy_threshold))))
    margins = {"gate": gate_margin, "det": det_margin, "prob": prob_margin}
    return unc, cost, np.stack([info[:, 0, 0], info[:, 0, 1], info[:, 1, 1]], axis=1), margins
