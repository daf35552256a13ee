"""TEST INFRASTRUCTURE: a pure-Python restatement of the obstacle logic of the EM planner's tree sampler, in the reference's own
form, on top of tests/em_tree_ref.py (which stays the restatement of everything else) -
  isSafe(node)            (src/em_exploration/Planner2D.cpp:48-56; Distance.cpp:78-97): unsafe iff an estimated landmark lies
                          strictly nearer than safe_distance; a negative radius finds nothing;
  sampleNode              (:101-125): Halton points until one is safe, every drawn point consumed; more than 1000 unsafe points end
                          the tree with SAMPLING_FAILURE;
  isSafe(node, parent)    (:58-86), asked by connectNode after the child is scaled (:243-248): |safe_distance| < 1e-3 is safe;
                          else d = range(child, parent), unit = the child's position in the PARENT's frame / d, and for
                          l = sd/2; l < d; l += sd/2 the point child.transform_from(l unit) - a point beyond the child, turned by the
                          child's heading, not a point between parent and child: the reference's behaviour as written, kept;
  the connect counter     (:1070-1079, :890-899): a refused connect adds no node, more than 1000 in a row end the tree;
  the shrink              (:1046-1054, :841-849): the call's safe_distance becomes distance - 0.1 (optimize2: not below 0) when the
                          current pose estimate is nearer than safe_distance to its nearest estimated landmark AND that landmark's
                          KEY is smaller than the NUMBER of landmarks (Simulator2D.cpp:394-403 returns the key, the planner compares
                          it with getLandmarkSize()); nearest in key order, strict <;
  rrt_planner's goal edge (:910-922): a goal whose edge is unsafe is not in the tree, the result is SUCCESS, the solution empty.
ONE DEVIATION, as the engine takes it: in rrt_planner a shrunk safe_distance below -1e-3 makes the reference's waypoint loop run
for ever (a negative step, l < d always true); the tree ends at once with SAMPLING_FAILURE, an empty plan, no point drawn.

Every run records what a test needs to know whether the case entitles it to exact comparisons: the rejected samples and edges, the
smallest |distance - safe_distance| over every safety comparison made (the gate margin), the smallest |d - l| over the l < d tests,
and the largest number of waypoints of an accepted edge."""
import math

import em_tree_ref as R
from em_tree_ref import SAMPLING_FAILURE, SUCCESS  # noqa: F401

MAX_FAILED = 1000   # `failed > 1000` of sampleNode and of the two growth loops
EDGE_EPS = 1e-3     # |safe_distance| below which isSafe(node, parent) tests nothing


class Stats(object):
    def __init__(self):
        self.rejected_samples = 0
        self.rejected_edges = 0
        self.gate_margin = float("inf")
        self.step_margin = float("inf")
        self.max_waypoints = 0      # of an accepted edge
        self.shrunk = False

    def gate(self, distance, sd):
        self.gate_margin = min(self.gate_margin, abs(distance - sd))


def point_is_safe(pt, landmarks, sd, stats=None):
    """isSafe(node): no landmark strictly nearer than sd (a negative radius finds nothing).  Every landmark is compared - only
    emptiness is asked, so the order does not matter - and every comparison enters the gate margin."""
    if sd < 0:
        return True
    safe = True
    for lm in landmarks:
        dx, dy = lm[0] - pt[0], lm[1] - pt[1]
        dist = math.sqrt(dx * dx + dy * dy)
        if stats is not None:
            stats.gate(dist, sd)
        if dist < sd:
            safe = False
    return safe


def waypoint_bound(max_edge_length):
    """The turns the waypoint loop can take: d <= max_edge_length (to rounding), the step sd/2 >= 5e-4."""
    return int(math.ceil(2.0 * max_edge_length / EDGE_EPS)) + 1


def waypoints(child, parent, sd, stats=None, bound=1 << 30):
    """The points isSafe(node, parent) tests, in order: child.transform_from(l unit), l = sd/2, sd, ... while l < d, l accumulated by
    repeated addition."""
    d = R.pose_range(child, (parent[0], parent[1]))
    dx, dy = child[0] - parent[0], child[1] - parent[1]
    lx, ly = parent[2] * dx + parent[3] * dy, -parent[3] * dx + parent[2] * dy  # pose2.transform_to(pose1.t())
    half = sd / 2
    out = []
    l = half
    while len(out) < bound:
        if stats is not None:
            stats.step_margin = min(stats.step_margin, abs(d - l))
        if not l < d:
            break
        inv = 1.0 / d
        ux, uy = inv * lx, inv * ly
        px, py = l * ux, l * uy
        out.append((child[0] + (child[2] * px - child[3] * py), child[1] + (child[3] * px + child[2] * py)))
        l += half
    return out


def edge_is_safe(child, parent, landmarks, sd, stats=None, point_safe=point_is_safe, bound=1 << 30):
    """isSafe(node, parent) for the non-Dubins control model; leaves at the first unsafe waypoint.  Returns (safe, waypoints passed)."""
    if abs(sd) < EDGE_EPS:
        return True, 0
    n = 0
    for w in waypoints(child, parent, sd, stats, bound):
        if not point_safe(w, landmarks, sd, stats):
            return False, n
        n += 1
    return True, n


def shrink(sd, root_xy, keys, landmarks, clamp, stats=None):
    """The safe_distance of one call.  `clamp`: optimize2's max(0, .); rrt_planner has none."""
    n = len(keys)
    if n == 0:
        return sd  # (searchLandmarkNearest answers 1, which is not below 0)
    best, nearest = float("inf"), -1
    for j in sorted(range(n), key=lambda q: keys[q]):  # the landmarks in key order, strict <
        dx, dy = landmarks[j][0] - root_xy[0], landmarks[j][1] - root_xy[1]
        dist = math.sqrt(dx * dx + dy * dy)
        if dist < best:
            best, nearest = dist, j
    if not int(keys[nearest]) < n:  # the KEY against the NUMBER of landmarks
        return sd
    if stats is not None:
        stats.gate(best, sd)
    if best < sd:
        if stats is not None:
            stats.shrunk = True
        return max(0.0, best - 0.1) if clamp else best - 0.1
    return sd


def child_of(origin, pt, max_edge_length):
    """connectNode's scaled child (Planner2D.cpp:188-216), before the edge test."""
    d = R.pose_range(origin, pt)
    angle = R.pose_bearing(origin, pt)
    length = max_edge_length if d > max_edge_length else d
    return R.compose(origin, R.make_pose(length * math.cos(angle), length * math.sin(angle), angle))


def grow(root_xytheta, bounds, angle_weight, max_edge_length, start, cap, keys, landmarks, safe_distance, n_accept=None, goal=None,
         point_safe=point_is_safe):
    """em_tree_ref.grow with the obstacle logic: the tree, with .stats, .sd (the call's safe_distance after the shrink).  keys,
    landmarks: the environment's estimated landmarks.  `point_safe` can be stubbed."""
    t = R.Tree(R.make_pose(*root_xytheta))
    st = t.stats = Stats()
    landmarks = [(float(p[0]), float(p[1])) for p in landmarks]
    sd = t.sd = shrink(safe_distance, (t.pose[0][0], t.pose[0][1]), keys, landmarks, goal is None, st)
    count = start
    t.halton_next = count
    if goal is not None and sd < -EDGE_EPS:  # the deviation: the reference would not return
        t.result = SAMPLING_FAILURE
        return t
    bound = waypoint_bound(max_edge_length)
    min_x, max_x, min_y, max_y = bounds
    failed = 0
    while True:
        if goal is None and len(t) - 1 >= n_accept:
            break
        if len(t) >= cap:
            t.result = SAMPLING_FAILURE if goal is not None else None
            break
        # sampleNode
        unsafe, pt = 0, None
        while pt is None:
            h = R.halton(count)
            count += 1
            p = (min_x + h[0] * (max_x - min_x), min_y + h[1] * (max_y - min_y))
            if point_safe(p, landmarks, sd, st):
                pt = p
            else:
                unsafe += 1
                st.rejected_samples += 1
                if unsafe > MAX_FAILED:
                    break
        if pt is None:
            t.result = SAMPLING_FAILURE
            break
        parent = t._nearest(pt, angle_weight)
        ok, n_way = edge_is_safe(child_of(t.pose[parent], pt, max_edge_length), t.pose[parent], landmarks, sd, st, point_safe, bound)
        if not ok:
            st.rejected_edges += 1
            failed += 1
            if failed > MAX_FAILED:
                t.result = SAMPLING_FAILURE
                break
            continue
        failed = 0
        st.max_waypoints = max(st.max_waypoints, n_way)
        node = t._connect(pt, parent, angle_weight, max_edge_length)
        if goal is not None:
            p = t.pose[node]
            if math.sqrt((p[0] - goal[0]) ** 2 + (p[1] - goal[1]) ** 2) <= max_edge_length:
                if len(t) >= cap:
                    t.result = SAMPLING_FAILURE
                    break
                ok, n_way = edge_is_safe(child_of(p, goal, max_edge_length), p, landmarks, sd, st, point_safe, bound)
                if ok:
                    t.goal_node = t._connect(goal, node, angle_weight, max_edge_length)
                else:
                    st.rejected_edges += 1
                    t.goal_edge_refused = True  # SUCCESS, the goal not in the tree, the solution empty
                break
    t.halton_next = count
    return t


def plan_leaves(t):
    """The leaves a finished optimize2 tree offers to the scoring: none after a sampling failure."""
    return t.leaves() if t.result == SUCCESS else []
