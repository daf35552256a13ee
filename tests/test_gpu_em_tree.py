"""GPU tests (run with -m gpu on an MI355X) of the EM planner's tree sampler - drlgx_em_plan / drlgx_rrt_plan
(csrc/k_em_tree.hip) and the facades over them - against tests/em_tree_ref.py on the beliefs, Halton start indices and tree sizes of
tests/em_tree_cases.py.  The restatement is run on the engine's own read-back belief (root pose, cell probabilities: inputs, not
results), and its nearest-node margins are asserted again here, which is what entitles these tests to EXACT parent indices.

Tolerance: node poses, distances and plan actions at the pose tolerance of DESIGN.md section 2, 1e-9 absolute (a chain of at most 40
composed fp64 poses at coordinates below 30 m stays orders of magnitude inside it).  The pick is compared bit for bit."""
import math
from configparser import ConfigParser

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_tree_cases as K  # noqa: E402
import em_tree_ref as R  # noqa: E402

ATOL = 1e-9
DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3


def make_engine(max_actions=K.MAX_ACTIONS):
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    cfg = default_config(K.MAP, num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES, max_actions=max_actions)
    eng = Engine(cfg, K.N_ENVS, 0)
    eng.reset(np.arange(K.N_ENVS), np.arange(K.N_ENVS), starts=K.STARTS)
    for act in K.SCRIPT:
        eng.step(torch.tensor([act] * K.N_ENVS, dtype=torch.float64, device=eng.device))
    assert eng.status() == 0
    return eng, cfg


class Ctx(object):
    def __init__(self):
        self.eng, self.cfg = make_engine()
        self.dev = self.eng.device
        self.root = [self.eng.poses(i)[0][-1] for i in range(K.N_ENVS)]
        self.known = [int(np.count_nonzero(self.eng.virtual_map(i)[0] < self.cfg.occupancy_threshold)) for i in range(K.N_ENVS)]
        self._trees = {}

    def i32(self, v):
        return torch.tensor(v, dtype=torch.int32, device=self.dev)

    def ref(self, env, start, n_accept):
        """The restatement's tree on the engine's own belief, computed once per case; its margins are asserted here again."""
        key = (env, start, n_accept)
        if key not in self._trees:
            t = K.tree_of(self.cfg, self.root[env], start, n_accept=n_accept)
            assert min(t.margin, default=1.0) > K.MARGIN
            self._trees[key] = t
        return self._trees[key]

    def live_state(self):
        out = []
        for i in range(K.N_ENVS):
            out += [self.eng.poses(i)[0], self.eng.poses(i)[1], self.eng.landmarks(i)[1], *self.eng.virtual_map(i)[:3]]
        return [np.array(a, copy=True) for a in out] + [self.eng.counts_dev().cpu().numpy()]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.eng.close()


def host(o):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def check_tree(nodes, n_nodes, t, tag):
    """Parents (hence depths and leaves) exact, poses / distances / edge odometry at 1e-9; returns the largest deviation."""
    assert n_nodes == len(t), tag
    nd = nodes[:n_nodes]
    np.testing.assert_array_equal(nd[:, 3].astype(np.int64), np.array(t.parent), err_msg=tag)
    xyt = t.xytheta()
    dth = np.abs(np.arctan2(np.sin(nd[:, 2] - xyt[:, 2]), np.cos(nd[:, 2] - xyt[:, 2])))
    dev = max(np.abs(nd[:, :2] - xyt[:, :2]).max(), dth.max(), np.abs(nd[:, 4] - np.array(t.distance)).max(),
              np.abs(nd[:, 5:8] - np.array(t.action)).max())
    assert dev <= ATOL, "%s: %.3e" % (tag, dev)
    return dev


def leaves_of(nodes, n_nodes):
    parent = nodes[:n_nodes, 3].astype(np.int64)
    has_child = np.zeros(n_nodes, dtype=bool)
    has_child[parent[1:]] = True
    return [j for j in range(n_nodes) if not has_child[j]], parent


def candidates_of(ctx, nodes, n_nodes, env):
    """The leaves of one tree as em_cost candidates, built from nodes_out alone: node order, edge odometry root -> leaf."""
    lv, parent = leaves_of(nodes, n_nodes)
    acts = np.zeros((len(lv), ctx.cfg.max_actions, 3))
    nact = np.zeros(len(lv), dtype=np.int32)
    for c, j in enumerate(lv):
        path = []
        while j > 0:
            path.insert(0, nodes[j, 5:8])
            j = parent[j]
        nact[c] = len(path)
        if path:
            acts[c, :len(path)] = np.array(path)
    return lv, torch.full((len(lv),), env, dtype=torch.int32, device=ctx.dev), torch.tensor(acts, device=ctx.dev), ctx.i32(nact)


@pytest.mark.parametrize("n_accept", K.NODE_COUNTS)
def test_topology_and_poses_match_the_restatement(ctx, n_accept):
    """Per environment its own max_nodes (so that max_nodes_ is exactly the size under test) and its own start index."""
    worst = 0.0
    for env in range(K.N_ENVS):
        start = K.START_INDICES[env]
        ctx.eng.set_sampler_parameter(K.max_nodes_for(ctx.known[env], n_accept))
        o = host(ctx.eng.em_plan(ctx.i32([env]), ctx.i32([start]), K.CAP, 0, want_nodes=True))
        assert ctx.eng.status() == 0
        t = ctx.ref(env, start, n_accept)
        tag = "env %d start %d nodes %d" % (env, start, n_accept)
        worst = max(worst, check_tree(o["nodes"][0], int(o["n_nodes"][0]), t, tag))
        assert int(o["result"][0]) == R.SUCCESS and int(o["halton_next"][0]) == start + n_accept == t.halton_next, tag
        lv, _ = leaves_of(o["nodes"][0], int(o["n_nodes"][0]))
        assert lv == t.leaves() and int(o["n_leaves"][0]) == len(lv), tag
        # the plan is one of the leaves' paths, in the layout em_cost reads, zero behind it
        na = int(o["n_actions"][0])
        paths = [t.actions_to(j) for j in t.leaves() if t.depth[j] == na]
        assert any(np.abs(np.array(p).reshape(-1, 3) - o["plan"][0, :na]).max(initial=0.0) <= ATOL for p in paths), tag
        assert np.all(o["plan"][0, na:] == 0.0), tag
        if n_accept == 0:
            assert na == 0 and lv == [0], tag
    print("nodes %d: largest deviation from the restatement %.3e" % (n_accept, worst))


@pytest.mark.parametrize("alg", [0, 1])
def test_pick_is_bit_equal_to_em_cost_on_the_leaves(ctx, alg):
    ctx.eng.set_sampler_parameter(K.max_nodes_for(ctx.known[0], 65))
    sel = ctx.i32(list(range(K.N_ENVS)))
    o = host(ctx.eng.em_plan(sel, ctx.i32(K.START_INDICES), K.CAP, alg, want_nodes=True))
    for env in range(K.N_ENVS):
        n_nodes = int(o["n_nodes"][env])
        assert n_nodes == R.max_nodes_of(ctx.eng.virtual_map(env)[0], ctx.cfg.occupancy_threshold, K.max_nodes_for(ctx.known[0], 65)) + 1
        lv, ce, acts, nact = candidates_of(ctx, o["nodes"][env], n_nodes, env)
        _, cost = ctx.eng.em_cost(ce, acts, nact, alg)
        cost = cost.cpu().numpy()
        best = R.pick(list(cost))
        assert len(lv) > 3 and len(set(cost)) > 1
        assert int(o["n_leaves"][env]) == len(lv)
        assert o["cost"][env] == cost[best]  # bit-equal
        assert int(o["n_actions"][env]) == int(nact[best])
        np.testing.assert_array_equal(o["plan"][env], acts[best].cpu().numpy())


def test_repeated_calls_are_bit_equal_live_state_untouched_and_halton_continues(ctx):
    ctx.eng.set_sampler_parameter(K.max_nodes_for(ctx.known[0], 20))
    sel = ctx.i32(list(range(K.N_ENVS)))
    before = ctx.live_state()
    a = host(ctx.eng.em_plan(sel, ctx.i32(K.START_INDICES), K.CAP, 0, want_nodes=True))
    b = host(ctx.eng.em_plan(sel, ctx.i32(K.START_INDICES), K.CAP, 0, want_nodes=True))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for x, y in zip(before, ctx.live_state()):
        np.testing.assert_array_equal(x, y)
    assert ctx.eng.status() == 0
    draws = a["n_nodes"] - 1
    np.testing.assert_array_equal(a["halton_next"], np.array(K.START_INDICES) + draws)
    c = host(ctx.eng.em_plan(sel, ctx.i32(a["halton_next"]), K.CAP, 0, want_nodes=True))
    for env in range(K.N_ENVS):
        t = K.tree_of(ctx.cfg, ctx.root[env], int(a["halton_next"][env]), n_accept=int(draws[env]))
        assert min(t.margin) > K.MARGIN
        check_tree(c["nodes"][env], int(c["n_nodes"][env]), t, "continued env %d" % env)


def run_plan(root, actions):
    p = R.make_pose(*root)
    for a in actions:
        p = R.compose(p, R.make_pose(*a))
    return p


def test_rrt_to_frontier_points_and_to_graph_nodes(ctx):
    sel = ctx.i32(list(range(K.N_ENVS)))
    none = ctx.i32([10 ** 6] * K.N_ENVS)  # (beyond key_size: the frontier point is the goal)
    goals = torch.tensor(K.RRT_GOALS, device=ctx.dev)
    o = host(ctx.eng.rrt_plan(sel, none, goals, ctx.i32(K.START_INDICES), K.CAP, want_nodes=True))
    assert ctx.eng.status() == 0
    for env in range(K.N_ENVS):
        t = K.tree_of(ctx.cfg, ctx.root[env], K.START_INDICES[env], goal=tuple(K.RRT_GOALS[env]))
        assert min(t.margin) > K.MARGIN and t.result == R.SUCCESS
        check_tree(o["nodes"][env], int(o["n_nodes"][env]), t, "rrt env %d" % env)
        na = int(o["n_actions"][env])
        assert int(o["result"][env]) == R.SUCCESS and na == t.depth[t.goal_node] and int(o["halton_next"][env]) == t.halton_next
        np.testing.assert_allclose(o["plan"][env, :na], np.array(t.actions_to(t.goal_node)), atol=ATOL)
        end = run_plan(ctx.root[env], o["plan"][env, :na])
        assert math.hypot(end[0] - K.RRT_GOALS[env][0], end[1] - K.RRT_GOALS[env][1]) <= ATOL
    # graph nodes as goals: landmark 1 (key order), pose 2, and a key beyond the graph (the frontier point again)
    counts = [ctx.eng.counts(i) for i in range(K.N_ENVS)]
    keys = [1, counts[1]["landmarks"] + 2, counts[2]["landmarks"] + counts[2]["poses"]]
    want = [ctx.eng.landmarks(0)[1][1], ctx.eng.poses(1)[0][2][:2], K.RRT_GOALS[2]]
    o = host(ctx.eng.rrt_plan(sel, ctx.i32(keys), goals, ctx.i32(K.START_INDICES), K.CAP, want_nodes=True))
    for env in range(K.N_ENVS):
        t = K.tree_of(ctx.cfg, ctx.root[env], K.START_INDICES[env], goal=tuple(want[env]))
        assert min(t.margin) > K.MARGIN and t.result == R.SUCCESS
        check_tree(o["nodes"][env], int(o["n_nodes"][env]), t, "rrt key env %d" % env)
        end = run_plan(ctx.root[env], o["plan"][env, :int(o["n_actions"][env])])
        assert math.hypot(end[0] - want[env][0], end[1] - want[env][1]) <= ATOL


def test_rrt_goal_beside_the_root_and_a_table_too_small(ctx):
    """A goal within one edge of the root.  The reference samples before it tests the goal (Planner2D.cpp:872-920: isReached is
    asked of the NEW node, never of the root), so the shortest tree is the root, one sampled node and the goal hung on it: two nodes
    beyond the root, a plan of two actions.  A table too small to reach a far goal ends with SAMPLING_FAILURE."""
    sel = ctx.i32(list(range(K.N_ENVS)))
    none = ctx.i32([-1] * K.N_ENVS)
    near = []
    for env, r in enumerate(ctx.root):  # 1.2 m from the root, 0.4 rad beside the first sample's direction: the first node (2 m that way) reaches it
        h = R.halton(K.START_INDICES[env])
        b = K.bounds(ctx.cfg)
        dx, dy = b[0] + h[0] * (b[1] - b[0]) - r[0], b[2] + h[1] * (b[3] - b[2]) - r[1]
        a = math.atan2(dy, dx) + 0.4  # (off the line through the root and that node: the bearing back to the goal is not +-pi)
        near.append([r[0] + 1.2 * math.cos(a), r[1] + 1.2 * math.sin(a)])
    near = np.array(near)
    o = host(ctx.eng.rrt_plan(sel, none, torch.tensor(near, device=ctx.dev), ctx.i32(K.START_INDICES), K.CAP, want_nodes=True))
    for env in range(K.N_ENVS):
        t = K.tree_of(ctx.cfg, ctx.root[env], K.START_INDICES[env], goal=tuple(near[env]))
        assert len(t) == 3 and t.parent == [-1, 0, 1]
        check_tree(o["nodes"][env], int(o["n_nodes"][env]), t, "near env %d" % env)
        assert int(o["n_actions"][env]) == 2 and int(o["result"][env]) == R.SUCCESS and int(o["halton_next"][env]) == K.START_INDICES[env] + 1
    far = torch.tensor(K.RRT_GOALS * 2.0, device=ctx.dev)
    o = host(ctx.eng.rrt_plan(sel, none, far, ctx.i32(K.START_INDICES), 6, want_nodes=True))
    assert ctx.eng.status() == 0
    for env in range(K.N_ENVS):
        t = K.tree_of(ctx.cfg, ctx.root[env], K.START_INDICES[env], goal=tuple(K.RRT_GOALS[env] * 2.0), cap=6)
        assert t.result == R.SAMPLING_FAILURE and len(t) == 6
        assert int(o["result"][env]) == R.SAMPLING_FAILURE and int(o["n_actions"][env]) == 0 and int(o["n_nodes"][env]) == 6
        assert np.all(o["plan"][env] == 0.0)


def test_rrt_goal_reached_by_the_node_that_fills_the_table(ctx):
    """The goals beside the root of the test above, whose full tree is the root, one node and the goal, in a table of two nodes: the
    node that reaches the goal has just filled the last slot, so the goal edge is not made (Planner2D.cpp has no table; the engine's
    is full): SAMPLING_FAILURE, the goal not connected, and everything up to there as with the full table."""
    sel = ctx.i32(list(range(K.N_ENVS)))
    none = ctx.i32([-1] * K.N_ENVS)
    near = []
    for env, r in enumerate(ctx.root):
        h = R.halton(K.START_INDICES[env])
        b = K.bounds(ctx.cfg)
        a = math.atan2(b[2] + h[1] * (b[3] - b[2]) - r[1], b[0] + h[0] * (b[1] - b[0]) - r[0]) + 0.4
        near.append([r[0] + 1.2 * math.cos(a), r[1] + 1.2 * math.sin(a)])
    near = torch.tensor(np.array(near), device=ctx.dev)
    whole = host(ctx.eng.rrt_plan(sel, none, near, ctx.i32(K.START_INDICES), K.CAP, want_nodes=True))
    o = host(ctx.eng.rrt_plan(sel, none, near, ctx.i32(K.START_INDICES), 2, want_nodes=True))
    assert ctx.eng.status() == 0
    for env in range(K.N_ENVS):
        tag = "env %d" % env
        t = K.tree_of(ctx.cfg, ctx.root[env], K.START_INDICES[env], goal=tuple(near[env].tolist()), cap=2)
        assert t.result == R.SAMPLING_FAILURE and len(t) == 2 and t.goal_node == -1, tag
        assert int(whole["n_nodes"][env]) == 3 and int(whole["result"][env]) == R.SUCCESS, tag
        assert int(o["result"][env]) == R.SAMPLING_FAILURE and int(o["n_nodes"][env]) == 2, tag
        assert int(o["n_actions"][env]) == 0 and np.all(o["plan"][env] == 0.0), tag
        assert int(o["halton_next"][env]) == int(whole["halton_next"][env]) == t.halton_next, tag
        np.testing.assert_array_equal(o["nodes"][env][:2], whole["nodes"][env][:2], err_msg=tag)
        check_tree(o["nodes"][env], 2, t, tag)


def error_code(call):
    from drl_graph_exploration_amd._lib import DrlgxError
    with pytest.raises(DrlgxError) as ei:
        call()
    return int(str(ei.value).split("drlgx error ")[1].split(":")[0])


def test_refusals_leave_the_status_word_and_the_live_state_alone(ctx):
    sel = ctx.i32(list(range(K.N_ENVS)))
    starts = ctx.i32(K.START_INDICES)
    # a non-zero safe_distance, the Dubins control model
    ctx.eng.set_sampler_parameter(0.1, safe_distance=1.0)
    assert error_code(lambda: ctx.eng.em_plan(sel, starts, K.CAP)) == DRLGX_E_INVALID
    assert error_code(lambda: ctx.eng.rrt_plan(sel, sel, torch.zeros(K.N_ENVS, 2, dtype=torch.float64, device=ctx.dev), starts, K.CAP)) == DRLGX_E_INVALID
    ctx.eng.set_sampler_parameter(0.1, dubins_control_model_enabled=True)
    assert error_code(lambda: ctx.eng.em_plan(sel, starts, K.CAP)) == DRLGX_E_INVALID
    # a tree that does not fit max_tree_nodes
    ctx.eng.set_sampler_parameter(K.max_nodes_for(ctx.known[0], 65))
    before = ctx.live_state()
    assert error_code(lambda: ctx.eng.em_plan(sel, starts, 20)) == DRLGX_E_CAPACITY
    assert ctx.eng.status() == 0
    # an engine with max_actions = 2 and a tree deeper than 2
    eng2, _ = make_engine(max_actions=2)
    try:
        t = K.tree_of(ctx.cfg, eng2.poses(0)[0][-1], 0, n_accept=65)
        assert max(t.depth) > 2
        known = int(np.count_nonzero(eng2.virtual_map(0)[0] < ctx.cfg.occupancy_threshold))
        eng2.set_sampler_parameter(K.max_nodes_for(known, 65))
        state = [np.array(a, copy=True) for a in (eng2.poses(0)[0], eng2.poses(0)[1], *eng2.virtual_map(0)[:3])]
        assert error_code(lambda: eng2.em_plan(ctx.i32([0]), ctx.i32([0]), K.CAP)) == DRLGX_E_CAPACITY
        assert eng2.status() == 0
        for x, y in zip(state, (eng2.poses(0)[0], eng2.poses(0)[1], *eng2.virtual_map(0)[:3])):
            np.testing.assert_array_equal(x, y)
    finally:
        eng2.close()
    for x, y in zip(before, ctx.live_state()):
        np.testing.assert_array_equal(x, y)


# Pose2 holds (cos, sin) as gtsam's does: .theta = atan2(sin theta, cos theta) is the angle to a few ulp of pi, not to the bit
THETA_ATOL = 1e-15


def same_odoms(got, want):
    np.testing.assert_array_equal(got[:, :2], want[:, :2])
    np.testing.assert_allclose(got[:, 2], want[:, 2], rtol=0, atol=THETA_ATOL)


def small_ini(lo, max_nodes):
    cp = ConfigParser()
    cp.read_dict({
        "Sensor Model": dict(bearing_noise="0.5", range_noise="0.02", min_bearing="-179.9", max_bearing="179.9", min_range="0.1", max_range="6.0"),
        "Control Model": dict(translation_noise="0.1", rotation_noise="0.2"),
        "Environment": dict(min_x="-6", max_x="6", min_y="-6", max_y="6", max_steps="5000", safe_distance="0.0"),
        "Virtual Map": dict(resolution="2.0", sigma0="1.0", num_samples="1"),
        "Simulator": dict(seed=str(lo), lo=str(lo), num=str(K.NUM_LANDMARKS), sigma_x0="0.05", sigma_y0="0.05", sigma_theta0="0.01"),
        "Planner": dict(seed=str(K.DEFAULT_SEED), angle_weight="0.4", distance_weight0="5.0", distance_weight1="2.0", d_weight="0.0",
                        max_edge_length="2.0", max_nodes=repr(max_nodes), occupancy_threshold="0.4", safe_distance="0.0", algorithm="EM_AOPT",
                        reg_out="false", dubins_control_model_enabled="false"),
    })
    return cp


def test_facades_agree_with_the_engine_call():
    """planner2d.EMPlanner2D.optimize2 / rrt_planner / iter_solution through the module classes, pyplanner2d.EMExplorer.plan() /
    rrt_plan() read as ExplorationEnv.plan / rrt_plan read them (edge.get_odoms()[0], inserted at the front), and
    VecExplorationEnv.em_plan(), each against Engine.em_plan / rrt_plan on the same belief."""
    from drl_graph_exploration_amd import planner2d
    from drl_graph_exploration_amd.pyplanner2d import EMExplorer
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    from staged_facade import StagedEMExplorer
    start = tuple(K.STARTS[0])
    h0 = planner2d.halton_start_index(K.DEFAULT_SEED)
    assert h0 == K.START_INDICES[1]
    for make in (StagedEMExplorer, EMExplorer):
        ex = make(small_ini(0, 0.2), start=start)
        for act in K.SCRIPT:
            ex.simulate(act)
        eng = ex.engine
        dev = eng.device
        sel, st = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([h0], dtype=torch.int32, device=dev)
        eng.set_sampler_parameter(0.2)
        want = host(eng.em_plan(sel, st, planner2d.EMPlanner2D.MAX_TREE_NODES, 0))
        na = int(want["n_actions"][0])
        assert na >= 1 and int(want["n_nodes"][0]) > 3
        if make is StagedEMExplorer:
            assert ex._planner.optimize2(ex._slam, ex._virtual_map) == planner2d.EMPlanner2D.OptimizationResult.SUCCESS
        else:
            assert ex.plan() is True
        edges = list(ex._planner.iter_solution())
        got = [[e.get_odoms()[0].x, e.get_odoms()[0].y, e.get_odoms()[0].theta] for e in edges]
        same_odoms(np.array(got), want["plan"][0, :na][::-1])  # leaf first: plan_out reversed
        actions = []
        for edge in ex._planner.iter_solution():  # (exploration_env.py:113-117)
            actions.insert(0, edge.get_odoms()[0].theta)
        np.testing.assert_allclose(actions, want["plan"][0, :na, 2], rtol=0, atol=THETA_ATOL)
        assert edges[-1].first.key == eng.counts(0)["poses"] - 1 and edges[0].second.key == edges[-1].first.key + na
        assert ex._planner.halton_next == int(want["halton_next"][0])
        # rrt to a frontier point, continuing the sequence
        goal = (float(K.RRT_GOALS[0][0]), float(K.RRT_GOALS[0][1]))
        st2 = torch.tensor([ex._planner.halton_next], dtype=torch.int32, device=dev)
        far = torch.tensor([10 ** 6], dtype=torch.int32, device=dev)
        rw = host(eng.rrt_plan(sel, far, torch.tensor([goal], dtype=torch.float64, device=dev), st2, planner2d.EMPlanner2D.MAX_TREE_NODES))
        if make is StagedEMExplorer:
            ok = ex._planner.rrt_planner(ex._slam, ex._virtual_map, 10 ** 6, goal[0], goal[1]) == planner2d.OptimizationResult.SUCCESS
        else:
            ok = ex.rrt_plan(10 ** 6, goal)
        assert ok and int(rw["result"][0]) == R.SUCCESS
        path = []
        for edge in ex._planner.iter_solution():  # (exploration_env.py:126-127)
            path.insert(0, edge.get_odoms()[0])
        same_odoms(np.array([[p.x, p.y, p.theta] for p in path]), rw["plan"][0, :int(rw["n_actions"][0])])
        if make is StagedEMExplorer:
            for name in ("optimize", "get_dubins_path", "iter_rrt"):
                with pytest.raises(NotImplementedError):
                    getattr(ex._planner, name)()
        eng.close()
    env = VecExplorationEnv(K.MAP, 2, env_index=0, test=True, starts=K.STARTS[:2], num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES,
                            n_rollouts=0)
    try:
        sel = torch.arange(2, dtype=torch.int32, device=env.device)
        env.engine.set_sampler_parameter(0.08)
        want = host(env.engine.em_plan(sel, torch.full((2,), h0, dtype=torch.int32, device=env.device), 2048, int(env.cfg.algorithm)))
        acts, n_act, result = env.em_plan(max_nodes=0.08)
        np.testing.assert_array_equal(acts.cpu().numpy(), want["plan"])
        np.testing.assert_array_equal(n_act.cpu().numpy(), want["n_actions"])
        assert (result.cpu().numpy() == R.SUCCESS).all()
        np.testing.assert_array_equal(env._halton_next.cpu().numpy(), want["halton_next"])
        gk = torch.full((2,), 10 ** 6, dtype=torch.int32, device=env.device)
        acts, n_act, result = env.rrt_plan(gk, torch.tensor(K.RRT_GOALS[:2], device=env.device))
        assert (result.cpu().numpy() == R.SUCCESS).all() and (n_act.cpu().numpy() >= 2).all()
    finally:
        env.close()
