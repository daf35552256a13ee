"""TEST INFRASTRUCTURE: a numpy / pure-Python restatement of the Dubins control model of the EM planner's tree sampler, in the
reference's own form, on top of tests/em_tree_ref.py (Halton, Pose2 algebra, nearestNode) and tests/em_safe_ref.py (isSafe(point),
the shrink, the retry loop of sampleNode) - by import, not by copy.  All citations are to src/em_exploration/Planner2D.cpp:
  the library             (:1359-1414): v from max_v while v > min_v - 1e-10 by v -= dv; w from 0 while w < max_w + 1e-10 by w += dw;
                          s = -1 then +1 (w = 0 is listed twice); from Pose2(0, 0, 0) and t = 0, while t < max_duration: num_steps++,
                          x += v dt cos, y += v dt sin, theta += s w dt through Pose2(x, y, theta) - the angle goes through (cos, sin)
                          and back through atan2 at every step -, t += dt, and an entry whenever t > min_duration (strict);
  sampleNode              (:41-45, :110-115): the generator has dimension 2 - the same x, y as em_tree_ref's -, theta = 0, unread;
  connectNodeDubinsPath   (:157-176): local = parent.transform_to(sample); the FIRST entry in library order with
                          |local - end_i| < tolerance_radius (strict) wins; the node's poses are num_steps Euler steps of that
                          (v, w) from the PARENT's pose; the node is the last of them;
  connectNode             (:179-265): no scaling, no bearing test; the library connect, then isSafe(node, parent);
                          key = parent.key + num_steps; distance = parent.distance + v dt n + |w dt n| angle_weight (:295-300);
  isSafe(node, parent)    (:59-70): safe at once if |safe_distance| < 1e-3, else poses 1 .. n - 2 each pass isSafe(point);
  rrt_planner             (:838-935): the shrink (unclamped), the sample retry loop, the connect counter of 1000 (which runs at
                          safe_distance = 0 too: a sample without a library path is a refused connect), isReached, and the goal edge
                          connectNode(goal, node) (:915): the goal joins only through a library path - else SUCCESS, an empty plan;
  Edge::getOdoms          (Planner2D.h:143-151): one odometry per step, origin.between(pose), the origin moving along.

Every run records what a test needs to know whether the case entitles it to exact comparisons: besides em_tree_ref's nearest-node
margins and em_safe_ref's gate margin, the smallest | |local - end_i| - tolerance_radius | over every entry the search had to decide
(all up to the winner; all of them when nothing matches), and how the matches fell over strides of 64 entries."""
import math

import numpy as np

import em_safe_ref as S
import em_tree_ref as R
from em_tree_ref import SAMPLING_FAILURE, SUCCESS  # noqa: F401

FIELDS = ("max_w", "dw", "min_v", "max_v", "dv", "dt", "min_duration", "max_duration", "tolerance_radius")


class Params(object):
    """EMPlanner2D::DubinsParameter."""

    def __init__(self, *values, **named):
        for f, v in zip(FIELDS, values):
            setattr(self, f, float(v))
        for f, v in named.items():
            setattr(self, f, float(v))

    def values(self):
        return [getattr(self, f) for f in FIELDS]


def step(pose, v, w, dt):
    """One Euler step through Pose2(x, y, theta): pose = (x, y, cos, sin)."""
    x = pose[0] + v * dt * pose[2]
    y = pose[1] + v * dt * pose[3]
    theta = math.atan2(pose[3], pose[2]) + w * dt
    return (x, y, math.cos(theta), math.sin(theta))


class Library(object):
    """The library in the reference's order: arrays v, w, num_steps, end [n, 3] (x, y, theta)."""

    def __init__(self, p):
        self.p = p
        v_, w_, n_, end = [], [], [], []
        v = p.max_v
        while v > p.min_v - 1e-10:
            w = 0.0
            while w < p.max_w + 1e-10:
                for s in (-1, 1):
                    t, ww = 0.0, w * s
                    pose, num_steps = (0.0, 0.0, 1.0, 0.0), 0
                    while t < p.max_duration:
                        num_steps += 1
                        pose = step(pose, v, ww, p.dt)
                        t += p.dt
                        if t > p.min_duration:
                            v_.append(v); w_.append(ww); n_.append(num_steps)
                            end.append((pose[0], pose[1], math.atan2(pose[3], pose[2])))
                w += p.dw
            v -= p.dv
        self.v, self.w = np.array(v_), np.array(w_)
        self.num_steps = np.array(n_, dtype=np.int64)
        self.end = np.array(end).reshape(-1, 3)
        self.dt, self.tol = p.dt, p.tolerance_radius

    def __len__(self):
        return len(self.v)

    def reach(self):
        """The largest |end|."""
        return float(np.sqrt(self.end[:, 0] ** 2 + self.end[:, 1] ** 2).max())


class Stats(S.Stats):
    def __init__(self):
        S.Stats.__init__(self)
        self.match_margin = float("inf")
        self.no_match = 0            # connects refused because no entry matched
        self.unsafe_path = 0         # connects refused by an unsafe intermediate pose
        self.drawn = 0               # Halton points drawn
        self.scanned = 0             # library entries the first-match search had to look at, in strides of 64
        self.multi_same_stride = 0   # accepted connects with a second match in the winner's stride of 64
        self.multi_other_stride = 0  # ... with a match in a later stride
        self.winners = []            # the library index of every accepted connect, the goal edge included
        self.tested_poses = 0
        self.unsafe_first_accepted = 0  # accepted paths whose first / last pose is unsafe (the reference tests neither)
        self.unsafe_last_accepted = 0


def match(lib, parent, pt, stats=None):
    """connectNodeDubinsPath's search: the first index whose end lies strictly within the tolerance radius of the point in the
    parent's frame, or -1."""
    dx, dy = pt[0] - parent[0], pt[1] - parent[1]
    lx, ly = parent[2] * dx + parent[3] * dy, -parent[3] * dx + parent[2] * dy
    ex, ey = lib.end[:, 0] - lx, lib.end[:, 1] - ly
    d = np.sqrt(ex * ex + ey * ey)
    hits = np.nonzero(d < lib.tol)[0]
    first = int(hits[0]) if len(hits) else -1
    if stats is not None:
        decided = d if first < 0 else d[:first + 1]
        stats.match_margin = min(stats.match_margin, float(np.abs(decided - lib.tol).min()))
        stats.scanned += len(lib) if first < 0 else min(len(lib), (first // 64 + 1) * 64)
        if first >= 0:
            stats.multi_same_stride += int(np.any(hits[1:] // 64 == first // 64))
            stats.multi_other_stride += int(np.any(hits[1:] // 64 > first // 64))
    return first


def path_poses(lib, m, parent):
    poses, pose = [], parent
    for _ in range(int(lib.num_steps[m])):
        pose = step(pose, float(lib.v[m]), float(lib.w[m]), lib.dt)
        poses.append(pose)
    return poses


def path_is_safe(poses, landmarks, sd, stats=None):
    """isSafe(node, parent) under the Dubins model: the first and the last pose are not tested; out at the first unsafe one."""
    if abs(sd) < S.EDGE_EPS:
        return True
    for i in range(1, len(poses) - 1):
        if stats is not None:
            stats.tested_poses += 1
        if not S.point_is_safe((poses[i][0], poses[i][1]), landmarks, sd, stats):
            return False
    return True


def edge_distance(lib, m, angle_weight):
    v, w, n = float(lib.v[m]), float(lib.w[m]), float(lib.num_steps[m])
    return v * lib.dt * n + abs(w * lib.dt * n) * angle_weight


def between(a, b):
    """Pose2::between as (x, y, theta)."""
    c, s = R._rot(a[2] * b[2] + a[3] * b[3], -a[3] * b[2] + a[2] * b[3])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return (a[2] * dx + a[3] * dy, -a[3] * dx + a[2] * dy, math.atan2(s, c))


def connect(t, lib, pt, parent, angle_weight, landmarks, sd):
    """connectNode(node, parent) under the Dubins model: the new node's index, or -1 when the connect is refused."""
    st = t.stats
    m = match(lib, t.pose[parent], pt, st)
    if m < 0:
        st.no_match += 1
        return -1
    poses = path_poses(lib, m, t.pose[parent])
    if not path_is_safe(poses, landmarks, sd, st):
        st.unsafe_path += 1
        return -1
    st.winners.append(m)
    if not abs(sd) < S.EDGE_EPS and len(poses) >= 2:  # (what the reference does not test: asked here without touching the margins)
        st.unsafe_first_accepted += not S.point_is_safe(poses[0][:2], landmarks, sd)
        st.unsafe_last_accepted += not S.point_is_safe(poses[-1][:2], landmarks, sd)
    t.pose.append(poses[-1])
    t.parent.append(parent)
    t.depth.append(t.depth[parent] + len(poses))        # in steps: key = parent.key + poses.size()
    t.distance.append(t.distance[parent] + edge_distance(lib, m, angle_weight))
    t.action.append((float(m), float(len(poses)), 0.0))  # the node's record: library index, num_steps, 0
    t.children.append(0)
    t.children[parent] += 1
    t.step_poses.append(poses)
    return len(t.pose) - 1


def grow(root_xytheta, bounds, angle_weight, max_edge_length, start, cap, lib, goal, keys=(), landmarks=(), safe_distance=0.0):
    """rrt_planner under the Dubins control model.  safe_distance = 0: no obstacle logic (the engine's plain instantiation); else
    the obstacle logic of em_safe_ref with rrt_planner's unclamped shrink.  The tree has .stats, .sd, .step_poses, .goal_edge_refused."""
    t = R.Tree(R.make_pose(*root_xytheta))
    st = t.stats = Stats()
    t.step_poses = [[]]
    t.goal_edge_refused = False
    landmarks = [(float(p[0]), float(p[1])) for p in landmarks]
    sd = t.sd = S.shrink(safe_distance, (t.pose[0][0], t.pose[0][1]), keys, landmarks, False, st) if safe_distance != 0 else 0.0
    count = start
    min_x, max_x, min_y, max_y = bounds
    failed = 0
    while True:
        if len(t) >= cap:
            t.result = SAMPLING_FAILURE
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
            t.result = SAMPLING_FAILURE
            break
        node = connect(t, lib, pt, t._nearest(pt, angle_weight), angle_weight, landmarks, sd)
        if node < 0:
            st.rejected_edges += 1
            failed += 1
            if failed > S.MAX_FAILED:
                t.result = SAMPLING_FAILURE
                break
            continue
        failed = 0
        p = t.pose[node]
        reach = math.sqrt((p[0] - goal[0]) ** 2 + (p[1] - goal[1]) ** 2)
        st.gate(reach, max_edge_length)  # (isReached is a decision too)
        if reach <= max_edge_length:
            if len(t) >= cap:
                t.result = SAMPLING_FAILURE
                break
            g = connect(t, lib, goal, node, angle_weight, landmarks, sd)
            if g >= 0:
                t.goal_node = g
            else:
                st.rejected_edges += 1
                t.goal_edge_refused = True
            break
    t.halton_next = count
    return t


def plan_rows(t):
    """Edge::getOdoms along the path root -> goal: one (x, y, theta) per step; [] without a goal node."""
    if t.goal_node < 0:
        return []
    path = [t.goal_node]
    while path[-1] > 0:
        path.append(t.parent[path[-1]])
    rows = []
    for node in reversed(path[:-1]):
        origin = t.pose[t.parent[node]]
        for pose in t.step_poses[node]:
            rows.append(between(origin, pose))
            origin = pose
    return rows
