"""TEST INFRASTRUCTURE: numpy restatements of the leaf evaluation with NON-CORE steps - the leaves of the Dubins control model
(src/em_exploration/Planner2D.cpp:652-737 updateNodeInformation_EM, :472-551 updateTrajectory_EM) - on top of oracle/fm2_ref.py,
tests/em_ref.py, tests/fm2_cases.py and tests/em_dubins_ref.py, by import:

  * fm2_update(sim, actions, core): every action appends a pose and its odometry factor (the chain cov1, F, Fs runs through every
    step, FastMarginals.cpp:201-223), only a core pose predicts measurements (:714-731: measured at node->state.pose, the edge's
    last pose).  The update term is applied to every pose's block (the reference applies it to `updated_keys` only - the old poses
    and each edge's last pose - and never reads the others).  core = all ones is oracle.fm2_ref.fm2_update.
  * information_form(sim, actions, core): the same posterior a second way - all odometry factors, the measurement factors of core
    poses only, blocks read off a Cholesky factor (fm2_cases.reference_information_form with the mask).
  * em_cost(sim, actions, core, distance): the leaf's map holds the old poses and the CORE new poses (:498, :514-524); the cost
    takes `distance` (the tree's, :293-303) when given.
  * grow(...): optimize2's growth loop (:1043-1092) over em_dubins_ref.connect - max_nodes_ accepted nodes, the connect counter
    of 1000, optimize2's clamped shrink - and leaf_candidates(tree): per leaf the per-step rows, the mask, the distance."""
import math

import numpy as np

import em_dubins_ref as D
import em_ref
import em_safe_ref as S
import em_tree_ref as R
import fm2_cases
from oracle import fm2_ref


def _gate(cfg, pose, xy):
    dx, dy = xy[0] - pose[0], xy[1] - pose[1]
    rng = math.sqrt(dx * dx + dy * dy)
    bearing = math.atan2(-pose[3] * dx + pose[2] * dy, pose[2] * dx + pose[3] * dy)
    return cfg.min_range < rng < cfg.max_range and cfg.min_bearing < bearing < cfg.max_bearing, rng, bearing


def _slot_landmarks(sim):
    keys, est, _ = sim.landmarks()
    slots = list(sim.slot_keys())
    out = np.zeros((len(slots), 2))
    for k, xy in zip(keys, est):
        out[slots.index(k)] = xy
    return out


def chain(sim, actions):
    """The predicted poses of the actions, chained from the last estimate as fm2_ref chains them."""
    origin = fm2_ref._pose(*sim.poses()[0][-1])
    out = []
    for a in actions:
        origin = fm2_ref._compose(origin, fm2_ref._pose(*a))
        out.append(origin)
    return out


def masked_counts(sim, actions, core):
    """(predicted measurements of core poses, of all poses, the smallest distance of a deciding pair from a gate)."""
    cfg, est = sim.cfg, _slot_landmarks(sim)
    masked = total = 0
    margin = math.inf
    for pose, c in zip(chain(sim, actions), core):
        for xy in est:
            seen, rng, bearing = _gate(cfg, pose, xy)
            total += seen
            if c:
                masked += seen
                margin = min(margin, abs(rng - cfg.max_range), abs(rng - cfg.min_range))
                if rng < cfg.max_range:
                    margin = min(margin, abs(bearing - cfg.max_bearing), abs(bearing - cfg.min_bearing))
    return int(masked), int(total), margin


def fm2_update(sim, actions, core):
    """fm2_ref.fm2_update with the mask: (cov [P + K, 3, 3], n_meas per new pose)."""
    cfg = sim.cfg
    Sig, L, P = sim.full_covariance()
    thp, _, thl, _, _ = sim.isam_state()
    est_lm = _slot_landmarks(sim)
    K = len(actions)
    sig = np.array([cfg.translation_noise, cfg.translation_noise, cfg.rotation_noise])
    sig_br = np.array([cfg.bearing_noise, cfg.range_noise])
    lidx = lambda j: slice(2 * j, 2 * j + 2)                      # noqa: E731
    pidx = lambda i: slice(2 * L + 3 * i, 2 * L + 3 * i + 3)      # noqa: E731
    origin, val0 = fm2_ref._pose(*sim.poses()[0][-1]), fm2_ref._pose(*thp[-1])
    new_pose, cov_new, Fs, F_ = [], [], [], []
    cov0, F = Sig[pidx(P - 1), pidx(P - 1)], np.eye(3)
    for a in actions:                                             # every step: FastMarginals.cpp:201-223
        odom = fm2_ref._pose(*a)
        end = fm2_ref._compose(origin, odom)
        new_pose.append(end)
        hx, H1b = fm2_ref._between(val0, end)
        h, _ = fm2_ref._between(odom, hx)
        Hl = np.array([[h[2], h[3], 0], [-h[3], h[2], 0], [0, 0, 1.0]])
        A0, A1 = (Hl @ H1b) / sig[:, None], Hl / sig[:, None]
        H1 = np.linalg.inv(A1)
        cov1 = H1 @ (A0 @ cov0 @ A0.T + np.eye(3)) @ H1.T
        F = -H1 @ A0 @ F
        Fs.append(F.copy()); F_.append(-H1 @ A0); cov_new.append(cov1)
        origin, val0, cov0 = end, end, cov1

    def _ix(k):
        return lidx(k[1]) if k[0] == "l" else pidx(k[1])

    def prop(k0, k1):                                             # FastMarginals2::propagate
        if k0 == k1:
            return cov_new[k0[1] - P] if k0[0] == "x" and k0[1] >= P else Sig[_ix(k0), _ix(k0)]
        new0, new1 = k0[0] == "x" and k0[1] >= P, k1[0] == "x" and k1[1] >= P
        if (new0 and not new1) or (new0 and new1 and k0[1] > k1[1]):
            return prop(k1, k0).T
        if new1:
            if not new0:
                return prop(k0, ("x", P - 1)) @ Fs[k1[1] - P].T
            return prop(k0, ("x", k1[1] - 1)) @ F_[k1[1] - P].T
        return Sig[_ix(k0), _ix(k1)]

    rows, n_meas = [], []
    for k, pose in enumerate(new_pose):
        cnt = 0
        if core[k]:                                               # measurements at core poses only
            for j in range(L):
                if _gate(cfg, pose, est_lm[j])[0]:
                    Jx, Jl = fm2_ref._br_jacobians(pose, thl[j])
                    rows.append((("x", P + k), ("l", j), Jx / sig_br[:, None], Jl / sig_br[:, None]))
                    cnt += 1
        n_meas.append(cnt)
    out = np.zeros((P + K, 3, 3))
    for i in range(P):
        out[i] = Sig[pidx(i), pidx(i)]
    for k in range(K):
        out[P + k] = cov_new[k]
    if not rows:
        return out, n_meas
    meas_keys = []
    for kx, kl, _, _ in rows:
        for kk in (kx, kl):
            if kk not in meas_keys:
                meas_keys.append(kk)
    col, c = {}, 0
    for kk in meas_keys:
        col[kk] = c
        c += 3 if kk[0] == "x" else 2
    cols, dim = c, 2 * len(rows)
    A = np.zeros((dim, cols))
    for r, (kx, kl, Jx, Jl) in enumerate(rows):
        A[2 * r:2 * r + 2, col[kx]:col[kx] + 3] = Jx
        A[2 * r:2 * r + 2, col[kl]:col[kl] + 2] = Jl
    SA = np.zeros((cols, cols))
    for k0 in meas_keys:
        for k1 in meas_keys:
            b = prop(k0, k1)
            SA[col[k0]:col[k0] + b.shape[0], col[k1]:col[k1] + b.shape[1]] = b
    Sm = A.T @ np.linalg.inv(np.eye(dim) + A @ SA @ A.T) @ A
    for i in range(P + K):
        Sg = np.zeros((3, cols))
        for kk in meas_keys:
            b = prop(("x", i), kk)
            Sg[:, col[kk]:col[kk] + b.shape[1]] = b
        out[i] += -Sg @ Sm @ Sg.T
    return out, n_meas


def information_form(sim, plan, core):
    """fm2_cases.reference_information_form with the mask: every odometry factor, the measurement factors of core poses only."""
    cfg = sim.cfg
    P, L, K = sim.num_poses(), sim.num_landmarks(), len(plan)
    thp, _, thl, _, _ = sim.isam_state()
    n0, n = 2 * L + 3 * P, 2 * L + 3 * (P + K)
    Lam = np.zeros((n, n))
    Lam[:n0, :n0] = fm2_cases.information_matrix(sim)
    px = lambda i: slice(2 * L + 3 * i, 2 * L + 3 * i + 3)   # noqa: E731
    sig = np.array([cfg.translation_noise, cfg.translation_noise, cfg.rotation_noise])
    sig_br = np.array([cfg.bearing_noise, cfg.range_noise])
    origin, val0 = fm2_ref._pose(*sim.poses()[0][-1]), fm2_ref._pose(*thp[-1])
    keys, est, _ = sim.landmarks()
    slot_of = {int(k): j for j, k in enumerate(sim.slot_keys())}
    for k, a in enumerate(plan):
        odom = fm2_ref._pose(*a)
        end = fm2_ref._compose(origin, odom)
        hx, H1b = fm2_ref._between(val0, end)
        h, _ = fm2_ref._between(odom, hx)
        Hl = np.array([[h[2], h[3], 0], [-h[3], h[2], 0], [0, 0, 1.0]])
        J = np.zeros((3, n))
        J[:, px(P + k - 1)], J[:, px(P + k)] = (Hl @ H1b) / sig[:, None], Hl / sig[:, None]
        Lam += J.T @ J
        if core[k]:
            for key, xy in zip(keys, est):
                if _gate(cfg, end, xy)[0]:
                    j = slot_of[int(key)]
                    Jx, Jl = fm2_ref._br_jacobians(end, thl[j])
                    J = np.zeros((2, n))
                    J[:, px(P + k)], J[:, 2 * j:2 * j + 2] = Jx / sig_br[:, None], Jl / sig_br[:, None]
                    Lam += J.T @ J
        origin, val0 = end, end
    return fm2_cases._pose_blocks(Lam, L, P + K)


def em_cost(sim, actions, core, distance=None, algorithm=0, cov=None):
    """em_ref.em_cost with the mask and the tree's distance: (uncertainty, cost, info [V, 3], touched [V] bool = the cells a pose
    of the leaf's map updated)."""
    cfg = sim.cfg
    actions = [tuple(float(v) for v in a) for a in actions]
    if cov is None:
        cov, _ = fm2_update(sim, actions, core)
    P = sim.num_poses()
    keep = [True] * P + [bool(c) for c in core[:len(actions)]]
    poses = em_ref.leaf_poses(sim, actions)[keep]                 # the chain composes every row; the map holds the core poses
    infos = np.array([np.linalg.inv(c) for c in cov[keep]])
    rows, cols = sim.vm_shape()
    info, upd, _, _ = em_ref.update_information(poses, infos, cfg, rows, cols)
    prob = sim.virtual_map()[0].reshape(-1)
    unc = em_ref.uncertainty(info, prob, algorithm)
    known = int(np.sum(prob < cfg.occupancy_threshold))
    dw = cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * (known / float(rows * cols))
    dist = em_ref.plan_distance(actions, cfg.angle_weight) if distance is None else float(distance)
    return unc, unc + dist * dw, np.stack([info[:, 0, 0], info[:, 0, 1], info[:, 1, 1]], axis=1), upd


def distance_weight(sim):
    cfg = sim.cfg
    prob = sim.virtual_map()[0].reshape(-1)
    return cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * (int(np.sum(prob < cfg.occupancy_threshold)) / float(prob.size))


# ------------------------------------------------------------------------------------------------ optimize2's tree under Dubins
def grow(root_xytheta, bounds, angle_weight, start, cap, lib, n_accept, keys=(), landmarks=(), safe_distance=0.0):
    """optimize2 under the Dubins control model: n_accept (= max_nodes_) accepted nodes, the connect counter of 1000 at any
    safe_distance, the sample retry loop and optimize2's clamped shrink under the obstacle logic.  The tree has .stats, .sd,
    .step_poses, .result, .halton_next, .full (the table filled first: the engine refuses the call)."""
    t = R.Tree(R.make_pose(*root_xytheta))
    st = t.stats = D.Stats()
    t.step_poses, t.full, t.result = [[]], False, R.SUCCESS
    landmarks = [(float(p[0]), float(p[1])) for p in landmarks]
    sd = t.sd = S.shrink(safe_distance, (t.pose[0][0], t.pose[0][1]), keys, landmarks, True, st) if safe_distance != 0 else 0.0
    count, failed = start, 0
    min_x, max_x, min_y, max_y = bounds
    while len(t) - 1 < n_accept:
        if len(t) >= cap:
            t.full = True
            break
        unsafe, pt = 0, None
        while pt is None:
            h = R.halton(count)
            count += 1
            st.drawn += 1
            p = (min_x + h[0] * (max_x - min_x), min_y + h[1] * (max_y - min_y))
            if safe_distance == 0 or S.point_is_safe(p, landmarks, sd, st):
                pt = p
            else:
                unsafe += 1
                st.rejected_samples += 1
                if unsafe > S.MAX_FAILED:
                    break
        if pt is None:
            t.result = R.SAMPLING_FAILURE
            break
        node = D.connect(t, lib, pt, t._nearest(pt, angle_weight), angle_weight, landmarks, sd)
        if node < 0:
            st.rejected_edges += 1
            failed += 1
            if failed > S.MAX_FAILED:
                t.result = R.SAMPLING_FAILURE
                break
            continue
        failed = 0
    t.halton_next = count
    return t


def leaf_candidates(t, max_actions):
    """What a finished tree hands to the scoring, per leaf in node order: (node, rows [K, 3], core [max_actions] u8, distance); none
    after a sampling failure."""
    out = []
    for node in (t.leaves() if t.result == R.SUCCESS else []):
        path = [node]
        while path[-1] > 0:
            path.append(t.parent[path[-1]])
        rows, core = [], np.zeros(max_actions, dtype=np.uint8)
        for j in reversed(path[:-1]):
            origin = t.pose[t.parent[j]]
            for pose in t.step_poses[j]:
                rows.append(D.between(origin, pose))
                origin = pose
            if len(rows) <= max_actions:
                core[len(rows) - 1] = 1
        out.append((node, np.array(rows).reshape(-1, 3), core, t.distance[node]))
    return out
