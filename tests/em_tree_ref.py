"""TEST INFRASTRUCTURE: a numpy / pure-Python restatement of the EM planner's tree sampler, in the reference's own form -
EMPlanner2D::initialize / sampleNode / nearestNode / connectNode and the stop rules of optimize2 and rrt_planner
(src/em_exploration/Planner2D.cpp:101-125, :188-276, :866-922, :1058-1111, :1281-1357), sqDistanceBetweenPoses / nearestNeighbor
(Distance.cpp:5-9, :24-35), the Halton sequence and the start index the planner's constructor draws (RNG.h:64-77,
Planner2D.cpp:36-45) - for the non-Dubins control model at safe_distance = 0.  Like tests/em_ref.py it has no reference vector:
tests/test_em_tree_cpu.py checks it by hand values before tests/test_gpu_em_tree.py uses it.

Poses are (x, y, cos, sin) as gtsam's Pose2 / Rot2 hold them.  Every nearest-node decision records its margin - the relative gap
between the best and the second-best distance - so that a test can tell whether a case entitles it to exact parent indices."""
import math

import numpy as np

SAMPLING_FAILURE, NO_SOLUTION, TERMINATION, SUCCESS = 0, 1, 2, 3


# ------------------------------------------------------------------ Halton, the start index
def radical_inverse(index, base):
    """sum_k d_k base^-(k+1) over all digits d_k of `index` in `base`."""
    f, r = 1.0, 0.0
    while index > 0:
        f = f / base
        r = r + f * (index % base)
        index //= base
    return r


def halton(index):
    """Halton point number `index` in three dimensions (bases 2, 3, 5)."""
    return radical_inverse(index, 2), radical_inverse(index, 3), radical_inverse(index, 5)


class MT19937(object):
    """The 32-bit Mersenne twister with the single-integer seeding (std::mt19937(seed))."""

    def __init__(self, seed=5489):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.idx = 624

    def _twist(self):
        mt = self.mt
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.idx = 0

    def next_u32(self):
        if self.idx >= 624:
            self._twist()
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF

    def canonical(self):
        """std::generate_canonical<double, 53>: two 32-bit outputs, the first the low part, over 2^64; below 1."""
        lo = self.next_u32()
        hi = self.next_u32()
        u = (float(lo) + float(hi) * 4294967296.0) / 18446744073709551616.0
        return u if u < 1.0 else math.nextafter(1.0, 0.0)


def start_index(seed):
    """qrng_.setCount(rng_.uniformInt(0, 100000)) of a planner constructed with `seed`: floor((high + 1 - low) u + low), clamped."""
    u = MT19937(seed).canonical()
    n = int(math.floor((100000 + 1.0 - 0.0) * u + 0.0))
    return min(max(n, 0), 100000)


# ------------------------------------------------------------------ Pose2 algebra (gtsam)
def _rot(c, s):
    if abs(c * c + s * s - 1.0) > 1e-9:
        n = math.sqrt(c * c + s * s)
        c, s = c / n, s / n
    return c, s


def make_pose(x, y, theta):
    return (x, y, math.cos(theta), math.sin(theta))


def compose(a, b):
    c, s = _rot(a[2] * b[2] - a[3] * b[3], a[3] * b[2] + a[2] * b[3])
    return (a[0] + (a[2] * b[0] - a[3] * b[1]), a[1] + (a[3] * b[0] + a[2] * b[1]), c, s)


def theta_of(p):
    return math.atan2(p[3], p[2])


def pose_range(p, pt):
    dx, dy = pt[0] - p[0], pt[1] - p[1]
    return math.sqrt(dx * dx + dy * dy)


def pose_bearing(p, pt):
    """Pose2::bearing(point).theta(): Rot2::relativeBearing of the point in the pose's frame."""
    dx, dy = pt[0] - p[0], pt[1] - p[1]
    lx, ly = p[2] * dx + p[3] * dy, -p[3] * dx + p[2] * dy
    n = math.sqrt(lx * lx + ly * ly)
    if abs(n) > 1e-5:
        c, s = _rot(lx / n, ly / n)
        return math.atan2(s, c)
    return 0.0


def sq_distance(p1, pt, angle_weight):
    """sqDistanceBetweenPoses(pose1, pose2, angle_weight) with pose2 at `pt` (Distance.cpp:5-9)."""
    return pose_range(p1, pt) ** 2 + (pose_bearing(p1, pt) * angle_weight) ** 2


# ------------------------------------------------------------------ the tree
class Tree(object):
    def __init__(self, root):
        self.pose = [root]
        self.parent = [-1]
        self.depth = [0]
        self.distance = [0.0]
        self.action = [(0.0, 0.0, 0.0)]
        self.children = [0]
        self.margin = []  # per draw: (second best - best) / max(best, tiny) of the nearest-node search (inf with one node)
        self.result = SUCCESS
        self.goal_node = -1
        self.halton_next = 0

    def __len__(self):
        return len(self.pose)

    def xytheta(self):
        return np.array([[p[0], p[1], theta_of(p)] for p in self.pose])

    def leaves(self):
        """The nodes without children, in node order (the root itself in a tree of one node)."""
        return [j for j in range(len(self)) if self.children[j] == 0]

    def actions_to(self, node):
        """The edge odometry root -> node."""
        out = []
        while node > 0:
            out.insert(0, self.action[node])
            node = self.parent[node]
        return out

    def _nearest(self, pt, angle_weight):
        d = [sq_distance(p, pt, angle_weight) for p in self.pose]
        n, best = -1, float("inf")  # (the reference starts from DBL_MAX: the same for finite distances)
        for i, di in enumerate(d):
            if di < best:
                best, n = di, i
        rest = [x for i, x in enumerate(d) if i != n]
        self.margin.append((min(rest) - best) / max(best, 1e-300) if rest else float("inf"))
        return n

    def _connect(self, pt, parent, angle_weight, max_edge_length):
        origin = self.pose[parent]
        d = pose_range(origin, pt)
        angle = pose_bearing(origin, pt)
        length = max_edge_length if d > max_edge_length else d
        act = (length * math.cos(angle), length * math.sin(angle), angle)
        child = compose(origin, make_pose(act[0], act[1], angle))
        self.pose.append(child)
        self.parent.append(parent)
        self.depth.append(self.depth[parent] + 1)
        self.distance.append(self.distance[parent] + math.sqrt(sq_distance(child, origin, angle_weight)))
        self.action.append(act)
        self.children.append(0)
        self.children[parent] += 1
        return len(self.pose) - 1


def max_nodes_of(prob, occupancy_threshold, max_nodes):
    """max_nodes_ = floor(#{p_v < occupancy_threshold} * max_nodes) (Planner2D.cpp:1322-1327)."""
    return int(math.floor(float(np.count_nonzero(np.asarray(prob) < occupancy_threshold)) * max_nodes))


def grow(root_xytheta, bounds, angle_weight, max_edge_length, start, cap, n_accept=None, goal=None):
    """One tree from the root pose: `n_accept` accepted nodes (optimize2) or until a node lies within max_edge_length of `goal`
    (rrt_planner), never more than `cap` nodes.  bounds = (min_x, max_x, min_y, max_y) of the map."""
    t = Tree(make_pose(*root_xytheta))
    count = start
    min_x, max_x, min_y, max_y = bounds
    while True:
        if goal is None and len(t) - 1 >= n_accept:
            break
        if len(t) >= cap:
            t.result = SAMPLING_FAILURE if goal is not None else None  # (None: optimize2's tree does not fit - a capacity refusal)
            break
        h = halton(count)
        count += 1
        pt = (min_x + h[0] * (max_x - min_x), min_y + h[1] * (max_y - min_y))  # (theta = 2 pi h[2] enters nothing at safe_distance 0)
        node = t._connect(pt, t._nearest(pt, angle_weight), angle_weight, max_edge_length)
        if goal is not None:
            p = t.pose[node]
            if math.sqrt((p[0] - goal[0]) ** 2 + (p[1] - goal[1]) ** 2) <= max_edge_length:
                if len(t) >= cap:
                    t.result = SAMPLING_FAILURE
                    break
                t.goal_node = t._connect(goal, node, angle_weight, max_edge_length)
                break
    t.halton_next = count
    return t


def pick(costs):
    """optimize2's choice over the leaves in node order (Planner2D.cpp:1110): the first is always taken, a later one only with a
    strictly smaller cost (a NaN never compares smaller)."""
    best = 0
    for k in range(1, len(costs)):
        if costs[k] < costs[best]:
            best = k
    return best
