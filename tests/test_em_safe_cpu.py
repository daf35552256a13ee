"""CPU tests of tests/em_safe_ref.py - the restatement of the tree sampler's obstacle logic that tests/test_gpu_em_safe.py is judged
against - by hand values, and of the conditions that entitle the GPU cases of tests/em_safe_cases.py to exact comparisons."""
import math

import numpy as np
import pytest

import em_safe_cases as SC
import em_safe_ref as S
import em_tree_cases as K
import em_tree_ref as R

BOX = (0.0, 8.0, 0.0, 9.0)


def test_waypoints_lie_beyond_the_child_not_between():
    """Parent at the origin heading 0, child scaled to 2 m at bearing 90 degrees: child (0, 2) heading 90 degrees.  The child in the
    parent's frame is (0, 2), unit (0, 1); child.transform_from(l (0, 1)) turns that by the child's heading: (0, 2) + l (-1, 0).  At
    safe_distance 1.5 the waypoints are l = 0.75 and 1.5: (-0.75, 2) and (-1.5, 2) - to the child's left, beyond it - where "between
    parent and child" would have been (0, 1.25) and (0, 0.5)."""
    parent = R.make_pose(0.0, 0.0, 0.0)
    child = S.child_of(parent, (0.0, 5.0), 2.0)
    np.testing.assert_allclose(child[:2], [0.0, 2.0], atol=1e-15)
    w = S.waypoints(child, parent, 1.5)
    np.testing.assert_allclose(w, [(-0.75, 2.0), (-1.5, 2.0)], atol=1e-15)
    # a landmark far to the right does not refuse the edge; one beside the child, to its left, does
    assert S.edge_is_safe(child, parent, [(3.0, 1.0)], 1.5) == (True, 2)
    assert S.edge_is_safe(child, parent, [(-1.0, 3.0)], 1.5) == (False, 0)
    # (0, 0.2) is 1.95 m from (-0.75, 2): safe there, and "between" would have met it at 0.3 m
    assert S.edge_is_safe(child, parent, [(0.0, 0.2)], 1.5) == (True, 2)
    # a parent with a heading: parent heading 90 degrees, sample straight ahead -> bearing 0, unit (1, 0), the waypoints run on ahead
    parent = R.make_pose(1.0, 1.0, math.pi / 2)
    child = S.child_of(parent, (1.0, 9.0), 2.0)
    np.testing.assert_allclose(S.waypoints(child, parent, 1.5), [(1.0, 3.75), (1.0, 4.5)], atol=1e-14)
    # |sd| < 1e-3 tests nothing; d = 0 makes no waypoint
    assert S.edge_is_safe(child, parent, [(1.0, 3.0)], 9e-4) == (True, 0)
    assert S.waypoints(parent, parent, 1.5) == []


def test_l_is_accumulated_and_the_comparison_is_strict():
    parent = R.make_pose(0.0, 0.0, 0.0)
    child = S.child_of(parent, (9.0, 0.0), 2.0)  # d = 2 exactly
    for sd in (0.5, 0.75, 1.0, 1.5, 3.0):  # half steps exact in binary: repeated addition = multiplication
        st = S.Stats()
        n = len(S.waypoints(child, parent, sd, st))
        assert n == len([k for k in range(1, 100) if k * (sd / 2) < 2.0])
    assert len(S.waypoints(child, parent, 1.0)) == 3  # 0.5, 1.0, 1.5; 2.0 < 2.0 is false
    assert len(S.waypoints(child, parent, 4.0)) == 0
    # repeated addition, not multiplication: 0.1 added ten times stays below 1, ten times 0.1 does not - a tenth waypoint
    short = S.child_of(parent, (1.0, 0.0), 2.0)
    acc = 0.0
    for _ in range(10):
        acc += 0.1
    assert acc < 1.0 and not 10 * 0.1 < 1.0
    assert len(S.waypoints(short, parent, 0.2)) == 10
    assert S.waypoint_bound(2.0) >= 4000


def test_point_safety_is_strict_and_a_negative_radius_finds_nothing():
    lms = [(3.0, 4.0)]
    assert S.point_is_safe((0.0, 0.0), lms, 5.0) is True   # at the distance exactly: not nearer
    assert S.point_is_safe((0.0, 0.0), lms, math.nextafter(5.0, 6.0)) is False
    assert S.point_is_safe((3.0, 4.0), lms, -1.0) is True
    assert S.point_is_safe((3.0, 4.0), lms, 0.0) is True
    assert S.point_is_safe((0.0, 0.0), [], 5.0) is True
    st = S.Stats()
    S.point_is_safe((0.0, 0.0), lms + [(0.0, 7.0)], 5.5, st)
    assert st.gate_margin == pytest.approx(0.5)


def test_both_shrink_rules_and_the_key_against_the_number_of_landmarks():
    lms = [(1.0, 0.0), (0.0, 3.0)]
    # nearest (1 m) has key 1 < 2 landmarks: the shrink applies
    assert S.shrink(1.5, (0.0, 0.0), [1, 0], lms, True) == pytest.approx(0.9)
    assert S.shrink(1.5, (0.0, 0.0), [1, 0], lms, False) == pytest.approx(0.9)
    assert S.shrink(0.8, (0.0, 0.0), [1, 0], lms, True) == 0.8            # not within safe_distance
    # key 2 is not below 2: no shrink, however near
    assert S.shrink(1.5, (0.0, 0.0), [2, 0], lms, True) == 1.5
    assert S.shrink(1.5, (0.0, 0.0), [5, 7], lms, False) == 1.5
    # within 0.1 m: optimize2 clamps at 0, rrt_planner goes negative
    assert S.shrink(1.5, (0.95, 0.0), [1, 0], lms, True) == 0.0
    assert S.shrink(1.5, (0.95, 0.0), [1, 0], lms, False) == pytest.approx(-0.05)
    # equal distances: the lower key is the nearest (key order, strict <) - here key 9 against key 0
    tie = [(1.0, 0.0), (-1.0, 0.0)]
    assert S.shrink(1.5, (0.0, 0.0), [9, 0], tie, True) == pytest.approx(0.9)
    assert S.shrink(1.5, (0.0, 0.0), [0, 9], tie, True) == pytest.approx(0.9)
    assert S.shrink(1.5, (0.0, 0.0), [9, 3], tie, True) == 1.5
    assert S.shrink(1.5, (0.0, 0.0), [], [], True) == 1.5


def grow(sd, lms, keys=None, **kw):
    keys = list(range(len(lms))) if keys is None else keys
    return S.grow((0.0, 0.0, 0.0), BOX, 0.4, 2.0, kw.pop("start", 1), kw.pop("cap", 16), keys, lms, sd, **kw)


def test_the_sample_counter():
    """Every point of the box unsafe: 1001 points are drawn and the tree ends; with one safe point after 1000 unsafe ones it goes on."""
    far = [(100.0, 100.0)]  # key 0 < 1, but 141 m away: within 500 -> the shrink would apply; use a key that is not below 1
    t = grow(500.0, far, keys=[1], n_accept=3)
    assert t.result == R.SAMPLING_FAILURE and len(t) == 1 and t.halton_next == 1 + 1001 and t.stats.rejected_samples == 1001
    assert S.plan_leaves(t) == []
    calls = []

    def stub(pt, lms, sd, stats=None):
        calls.append(pt)
        return len(calls) >= 1001  # 1000 unsafe points, then everything safe

    t = grow(1.0, [], n_accept=1, point_safe=stub)
    assert t.result == R.SUCCESS and len(t) == 2 and t.halton_next == 1 + 1001 and t.stats.rejected_samples == 1000


def test_the_connect_counter_at_1000_and_1001():
    """A stubbed predicate: samples (the points of the Halton sequence) are safe, waypoints (anything else) are not, for the first
    `n_bad` edges."""
    def run(n_bad, **kw):
        state = {"edges": 0}
        samples = set()
        for k in range(1, 1200):
            h = R.halton(k)
            samples.add((BOX[0] + h[0] * (BOX[1] - BOX[0]), BOX[2] + h[1] * (BOX[3] - BOX[2])))

        def stub(pt, lms, sd, stats=None):
            if pt in samples:
                return True
            state["edges"] += 1
            return state["edges"] > n_bad
        # (the root outside the box: every edge from it is scaled to 2 m and has waypoints to ask the predicate about)
        return S.grow((-10.0, -10.0, 0.0), BOX, 0.4, 2.0, 1, 16, [0], [(50.0, 50.0)], 1.0, point_safe=stub, **kw)
    t = run(1000, n_accept=2)
    assert t.result == R.SUCCESS and len(t) == 3 and t.stats.rejected_edges == 1000
    t = run(1001, n_accept=2)
    assert t.result == R.SAMPLING_FAILURE and len(t) == 1 and t.stats.rejected_edges == 1001 and t.halton_next == 1 + 1001
    t = run(1001, goal=(7.5, 8.5))
    assert t.result == R.SAMPLING_FAILURE and len(t) == 1 and t.goal_node == -1
    # an accepted edge resets the counter: 600 edges refused, one accepted (its three waypoints pass), 600 refused again, then all
    # pass - more than 1000 refusals in all, never more than 600 in a row
    state = {"n": 0}

    def in_two_runs(pt, lms, sd, stats=None):
        state["n"] += 1
        return 600 < state["n"] <= 603 or state["n"] > 1203

    t = S.grow((-10.0, -10.0, 0.0), BOX, 0.4, 2.0, 1, 16, [], [], 1.0, n_accept=2, point_safe=lambda p, l, s, st=None: True)
    assert len(S.waypoints(t.pose[1], t.pose[0], 1.0)) == 3

    samples = {(BOX[0] + R.halton(k)[0] * (BOX[1] - BOX[0]), BOX[2] + R.halton(k)[1] * (BOX[3] - BOX[2])) for k in range(1, 1300)}
    t = S.grow((-10.0, -10.0, 0.0), BOX, 0.4, 2.0, 1, 16, [], [], 1.0, n_accept=2,
               point_safe=lambda p, l, s, st=None: True if p in samples else in_two_runs(p, l, s, st))
    assert t.result == R.SUCCESS and len(t) == 3 and t.stats.rejected_edges > 1000


def test_the_rrt_goal_edge_and_the_deviation():
    """Hand tree of em_tree_ref's CPU test: root (0, 0, 0), Halton point 1 = (4, 3) -> node 1 at (1.6, 1.2) heading atan2(3, 4); the
    goal (2.5, 2.5) is within 2 m of it.  The goal child sits on the goal with heading = bearing 1 + bearing 2; its waypoints run
    beyond it.  A landmark there refuses the goal edge: SUCCESS, no goal node, an empty solution."""
    free = grow(1.0, [(-30.0, -30.0)], goal=(2.5, 2.5))
    assert free.parent == [-1, 0, 1] and free.goal_node == 2 and free.result == R.SUCCESS
    node, goal_pose = free.pose[1], free.pose[2]
    w = S.waypoints(goal_pose, node, 1.0)
    assert len(w) >= 1
    lm = (w[-1][0], w[-1][1] + 0.3)  # 0.3 m from the last waypoint
    assert S.edge_is_safe(free.pose[1], free.pose[0], [lm], 1.0)[0]  # the first edge stays safe
    t = grow(1.0, [lm, (-30.0, -30.0)], keys=[5, 6], goal=(2.5, 2.5))
    assert t.result == R.SUCCESS and t.goal_node == -1 and t.parent == [-1, 0] and t.goal_edge_refused and t.halton_next == 2
    # the deviation: the root 0.05 m from a landmark whose key is below the count -> rrt_planner's safe_distance is -0.05
    t = grow(1.0, [(0.05, 0.0)], goal=(2.5, 2.5), start=17)
    assert t.sd == pytest.approx(-0.05) and t.result == R.SAMPLING_FAILURE and len(t) == 1 and t.halton_next == 17 and t.goal_node == -1
    # optimize2 clamps at 0 instead and grows the plain tree
    t = grow(1.0, [(0.05, 0.0)], n_accept=3, start=17)
    assert t.sd == 0.0 and t.result == R.SUCCESS and len(t) == 4
    # between -1e-3 and 0 the reference's loop is not entered (|sd| < 1e-3) and a negative radius finds nothing: the plain tree
    t = grow(1.0, [(0.0995, 0.0)], goal=(2.5, 2.5))
    assert -1e-3 < t.sd < 0 and t.result == R.SUCCESS and t.parent == free.parent


def same_tree(a, b):
    assert a.pose == b.pose and a.parent == b.parent and a.depth == b.depth and a.distance == b.distance and a.action == b.action
    assert a.children == b.children and a.margin == b.margin and a.result == b.result and a.goal_node == b.goal_node
    assert a.halton_next == b.halton_next


def test_at_safe_distance_zero_the_restatement_is_em_tree_ref_exactly():
    sims = K.make_sims()
    for i, sim in enumerate(sims):
        root = sim.poses()[0][-1]
        keys, xy, _ = sim.landmarks()
        for start in K.START_INDICES:
            same_tree(SC.tree_of(sim.cfg, root, keys, xy, 0.0, start, n_accept=65, cap=K.CAP), K.tree_of(sim.cfg, root, start, n_accept=65))
        same_tree(SC.tree_of(sim.cfg, root, keys, xy, 0.0, K.START_INDICES[i], goal=tuple(K.RRT_GOALS[i]), cap=K.CAP),
                  K.tree_of(sim.cfg, root, K.START_INDICES[i], goal=tuple(K.RRT_GOALS[i])))
    same_tree(S.grow((0.0, 0.0, 0.0), BOX, 0.4, 2.0, 1, 2, [], [], 0.0, goal=(7.5, 8.5)), R.grow((0.0, 0.0, 0.0), BOX, 0.4, 2.0, 1, 2, goal=(7.5, 8.5)))


def test_the_gpu_cases_meet_their_conditions_on_the_oracles_beliefs():
    """What tests/test_gpu_em_safe.py asserts again on the engine's own beliefs: rejections in every environment, an accepted edge with
    two waypoints, every margin above 1e-9; the goals whose edge is refused; set B's shrinks and failures."""
    sims = K.make_sims()
    for i, sim in enumerate(sims):
        root, (keys, xy, _) = sim.poses()[0][-1], sim.landmarks()
        t = SC.tree_of(sim.cfg, root, keys, xy, SC.SAFE_DISTANCE, K.START_INDICES[i], n_accept=SC.N_ACCEPT)
        assert t.result == R.SUCCESS and len(t) == SC.N_ACCEPT + 1 and max(t.depth) <= K.MAX_ACTIONS and SC.entitled(t)
        assert t.stats.rejected_samples >= 1 and t.stats.rejected_edges >= 1 and t.stats.max_waypoints >= 2 and not t.stats.shrunk
        g = SC.tree_of(sim.cfg, root, keys, xy, SC.SAFE_DISTANCE, K.START_INDICES[i], goal=tuple(K.RRT_GOALS[i]))
        assert g.result == R.SUCCESS and g.goal_node > 0 and SC.entitled(g)
        u = SC.tree_of(sim.cfg, root, keys, xy, SC.SAFE_DISTANCE, K.START_INDICES[i], goal=tuple(SC.UNSAFE_GOALS[i]))
        assert u.result == R.SUCCESS and u.goal_node == -1 and u.goal_edge_refused and len(u) < SC.CAP and SC.entitled(u)
    b = SC.make_sims_b()
    bel = [(s.cfg, s.poses()[0][-1], *s.landmarks()[:2]) for s in b]
    for i, (cfg, root, keys, xy) in enumerate(bel):
        d = np.hypot(xy[:, 0] - root[0], xy[:, 1] - root[1])
        order = np.argsort(keys)
        nearest = order[np.argmin(d[order])]
        assert (keys[nearest] >= len(keys)) == (i in (SC.B_KEY_HIGH, SC.B_WALLED))
        if i == SC.B_NEAR:
            assert keys[nearest] == 0 and d[nearest] < 0.099
        if i == SC.B_KEY_HIGH:
            assert d[nearest] < SC.SHRINK_DISTANCE
    cfg, root, keys, xy = bel[SC.B_NEAR]
    t = SC.tree_of(cfg, root, keys, xy, SC.SHRINK_DISTANCE, SC.B_START_INDEX, n_accept=SC.B_ACCEPT)
    assert t.sd == 0.0 and t.stats.shrunk and t.result == R.SUCCESS
    t = SC.tree_of(cfg, root, keys, xy, SC.SHRINK_DISTANCE, SC.B_START_INDEX, goal=tuple(SC.B_RRT_GOALS[SC.B_NEAR]))
    assert t.sd < -1e-3 and t.result == R.SAMPLING_FAILURE and len(t) == 1 and t.halton_next == SC.B_START_INDEX
    cfg, root, keys, xy = bel[SC.B_KEY_HIGH]
    for kw in (dict(n_accept=SC.B_ACCEPT), dict(goal=tuple(SC.B_RRT_GOALS[SC.B_KEY_HIGH]))):
        t = SC.tree_of(cfg, root, keys, xy, SC.SHRINK_DISTANCE, SC.B_START_INDEX, **kw)
        assert t.sd == SC.SHRINK_DISTANCE and not t.stats.shrunk and t.result == R.SUCCESS and SC.entitled(t) and t.stats.rejected_edges >= 1
        t = SC.tree_of(cfg, root, keys, xy, SC.FAIL_DISTANCE, SC.B_START_INDEX, **kw)
        assert t.result == R.SAMPLING_FAILURE and len(t) == 1 and t.halton_next == SC.B_START_INDEX + 1001 and t.stats.gate_margin > 1.0
    cfg, root, keys, xy = bel[SC.B_PLAIN]
    for sd in (SC.SHRINK_DISTANCE, SC.FAIL_DISTANCE, SC.WALLED_DISTANCE):
        t = SC.tree_of(cfg, root, keys, xy, sd, SC.B_START_INDEX, n_accept=SC.B_ACCEPT)
        assert 0.5 < t.sd < 2.0 and t.stats.shrunk and t.result == R.SUCCESS and SC.entitled(t)
    cfg, root, keys, xy = bel[SC.B_WALLED]
    for kw in (dict(n_accept=SC.B_ACCEPT), dict(goal=tuple(SC.B_RRT_GOALS[SC.B_WALLED]))):
        t = SC.tree_of(cfg, root, keys, xy, SC.WALLED_DISTANCE, SC.B_START_INDEX, **kw)
        assert t.result == R.SAMPLING_FAILURE and len(t) == 1 and t.stats.rejected_edges == 1001 and SC.entitled(t)
        assert t.halton_next == SC.B_START_INDEX + 1001 + t.stats.rejected_samples
