"""GPU tests (run with -m gpu on an MI355X) of the tree sampler's obstacle logic - the kSafe instantiation of k_em_tree
(csrc/k_em_tree.hip) behind Engine.set_sampler_obstacles - against tests/em_safe_ref.py on the cases of tests/em_safe_cases.py.  As in
tests/test_gpu_em_tree.py the restatement runs on the engine's own read-back belief (root pose, landmark keys and estimates, cell
probabilities: inputs, not results), and the margins that entitle a case to exact comparisons - nearest-node, gate and step margins -
are asserted here again on that belief.

Exact: parents (hence depths and leaves), n_nodes, halton_next, result, the leaf list, the pick.  Node poses, distances and edge
odometry at the pose tolerance of tests/test_gpu_em_tree.py, 1e-9 absolute."""
from configparser import ConfigParser

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_safe_cases as SC  # noqa: E402
import em_tree_cases as K  # noqa: E402
import em_tree_ref as R  # noqa: E402

ATOL = 1e-9
THETA_ATOL = 1e-15
DRLGX_E_INVALID = -1


class Ctx(object):
    """One engine, its beliefs read back once."""

    def __init__(self, seeds, starts, fixed=None):
        from drl_graph_exploration_amd import default_config
        from drl_graph_exploration_amd.engine import Engine
        self.n = len(seeds)
        self.cfg = default_config(K.MAP, num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES, max_actions=K.MAX_ACTIONS)
        self.eng = Engine(self.cfg, self.n, 0)
        self.eng.set_sampler_obstacles(True)  # (without the feature every test of this file fails here)
        if fixed:
            self.eng.set_fixed_landmarks(fixed)
        self.eng.reset(np.arange(self.n), np.array(seeds), starts=np.array(starts))
        for act in K.SCRIPT:
            self.eng.step(torch.tensor([act] * self.n, dtype=torch.float64, device=self.eng.device))
        assert self.eng.status() == 0
        self.dev = self.eng.device
        self.root = [self.eng.poses(i)[0][-1] for i in range(self.n)]
        self.lm = [self.eng.landmarks(i)[:2] for i in range(self.n)]
        self.known = [int(np.count_nonzero(self.eng.virtual_map(i)[0] < self.cfg.occupancy_threshold)) for i in range(self.n)]
        self._trees = {}

    def i32(self, v):
        return torch.tensor(v, dtype=torch.int32, device=self.dev)

    def f64(self, v):
        return torch.tensor(np.asarray(v, dtype=np.float64), device=self.dev)

    def ref(self, env, sd, start, n_accept=None, goal=None, cap=SC.CAP):
        key = (env, sd, start, n_accept, None if goal is None else tuple(goal), cap)
        if key not in self._trees:
            keys, xy = self.lm[env]
            self._trees[key] = SC.tree_of(self.cfg, self.root[env], keys, xy, sd, start, n_accept=n_accept,
                                          goal=None if goal is None else tuple(goal), cap=cap)
        return self._trees[key]

    def sampler(self, env, n_accept, sd):
        self.eng.set_sampler_parameter(K.max_nodes_for(self.known[env], n_accept), safe_distance=sd)

    def live_state(self):
        out = []
        for i in range(self.n):
            out += [self.eng.poses(i)[0], self.eng.poses(i)[1], self.eng.landmarks(i)[1], *self.eng.virtual_map(i)[:3]]
        return [np.array(a, copy=True) for a in out] + [self.eng.counts_dev().cpu().numpy()]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx(list(range(K.N_ENVS)), K.STARTS)
    yield c
    c.eng.close()


@pytest.fixture(scope="module")
def ctxb():
    c = Ctx(SC.B_SEEDS, SC.B_STARTS, fixed=SC.FIXED)
    yield c
    c.eng.close()


def host(o):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def check_tree(nodes, n_nodes, t, tag):
    """tests/test_gpu_em_tree.py's criteria: parents exact, poses / distances / edge odometry at 1e-9."""
    assert n_nodes == len(t), tag
    nd = nodes[:n_nodes]
    np.testing.assert_array_equal(nd[:, 3].astype(np.int64), np.array(t.parent), err_msg=tag)
    xyt = t.xytheta()
    dth = np.abs(np.arctan2(np.sin(nd[:, 2] - xyt[:, 2]), np.cos(nd[:, 2] - xyt[:, 2])))
    dev = max(np.abs(nd[:, :2] - xyt[:, :2]).max(), dth.max(), np.abs(nd[:, 4] - np.array(t.distance)).max(),
              np.abs(nd[:, 5:8] - np.array(t.action)).max())
    assert dev <= ATOL, "%s: %.3e" % (tag, dev)


def leaves_of(nodes, n_nodes):
    parent = nodes[:n_nodes, 3].astype(np.int64)
    has_child = np.zeros(n_nodes, dtype=bool)
    has_child[parent[1:]] = True
    return [j for j in range(n_nodes) if not has_child[j]], parent


def check_pick(c, o, row, env, alg=0):
    """The plan is the first leaf with the strictly smallest em_cost, bit for bit (the leaves as candidates from nodes_out alone)."""
    nodes, n_nodes = o["nodes"][row], int(o["n_nodes"][row])
    lv, parent = leaves_of(nodes, n_nodes)
    acts = np.zeros((len(lv), c.cfg.max_actions, 3))
    nact = np.zeros(len(lv), dtype=np.int32)
    for k, j in enumerate(lv):
        path = []
        while j > 0:
            path.insert(0, nodes[j, 5:8])
            j = parent[j]
        nact[k] = len(path)
        if path:
            acts[k, :len(path)] = np.array(path)
    _, cost = c.eng.em_cost(torch.full((len(lv),), env, dtype=torch.int32, device=c.dev), c.f64(acts), c.i32(nact), alg)
    cost = cost.cpu().numpy()
    best = R.pick(list(cost))
    assert int(o["n_leaves"][row]) == len(lv) and o["cost"][row] == cost[best] and int(o["n_actions"][row]) == int(nact[best])
    np.testing.assert_array_equal(o["plan"][row], acts[best])
    return lv


def check_failed(o, row, n_nodes, halton_next, tag):
    assert int(o["result"][row]) == R.SAMPLING_FAILURE and int(o["n_nodes"][row]) == n_nodes, tag
    assert int(o["n_actions"][row]) == 0 and np.all(o["plan"][row] == 0.0) and int(o["halton_next"][row]) == halton_next, tag
    if "n_leaves" in o:
        assert int(o["n_leaves"][row]) == 0, tag


def rrt(c, sel, goals, starts, cap=SC.CAP):
    none = c.i32([10 ** 6] * len(sel))  # (beyond key_size: the point is the goal)
    return host(c.eng.rrt_plan(c.i32(sel), none, c.f64(goals), c.i32(starts), cap, want_nodes=True))


# ---------------------------------------------------------------- 1
def test_opted_in_at_safe_distance_zero_is_bit_equal_to_the_plain_call(ctx):
    sel, starts = ctx.i32(list(range(K.N_ENVS))), ctx.i32(K.START_INDICES)
    goals = ctx.f64(K.RRT_GOALS)
    none = ctx.i32([10 ** 6] * K.N_ENVS)
    ctx.sampler(0, 65, 0.0)
    try:
        on = host(ctx.eng.em_plan(sel, starts, K.CAP, 0, want_nodes=True)), host(ctx.eng.rrt_plan(sel, none, goals, starts, K.CAP, want_nodes=True))
        ctx.eng.set_sampler_obstacles(False)
        off = host(ctx.eng.em_plan(sel, starts, K.CAP, 0, want_nodes=True)), host(ctx.eng.rrt_plan(sel, none, goals, starts, K.CAP, want_nodes=True))
    finally:
        ctx.eng.set_sampler_obstacles(True)
    for a, b in zip(on, off):
        assert int(a["n_nodes"].min()) > 3
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert ctx.eng.status() == 0


# ---------------------------------------------------------------- 2
def test_trees_under_obstacles_match_the_restatement(ctx):
    sd = SC.SAFE_DISTANCE
    two_waypoints = 0
    for env in range(K.N_ENVS):
        start = K.START_INDICES[env]
        t = ctx.ref(env, sd, start, n_accept=SC.N_ACCEPT)
        # what makes the comparison meaningful, on the restatement alone
        assert t.stats.rejected_samples >= 1 and t.stats.rejected_edges >= 1, env
        assert SC.entitled(t), (env, min(t.margin), t.stats.gate_margin, t.stats.step_margin)
        two_waypoints += t.stats.max_waypoints >= 2
        ctx.sampler(env, SC.N_ACCEPT, sd)
        o = host(ctx.eng.em_plan(ctx.i32([env]), ctx.i32([start]), SC.CAP, 0, want_nodes=True))
        assert ctx.eng.status() == 0
        tag = "env %d" % env
        check_tree(o["nodes"][0], int(o["n_nodes"][0]), t, tag)
        assert int(o["result"][0]) == t.result == R.SUCCESS and int(o["halton_next"][0]) == t.halton_next, tag
        assert t.halton_next == start + SC.N_ACCEPT + t.stats.rejected_samples + t.stats.rejected_edges, tag
        assert check_pick(ctx, o, 0, env) == t.leaves(), tag
        print("env %d: %d samples and %d edges refused, gate margin %.2e, step margin %.2e" % (
            env, t.stats.rejected_samples, t.stats.rejected_edges, t.stats.gate_margin, t.stats.step_margin))
    assert two_waypoints >= 1
    # rrt_planner under the same obstacles, all trees in one call
    o = rrt(ctx, list(range(K.N_ENVS)), K.RRT_GOALS, K.START_INDICES)
    for env in range(K.N_ENVS):
        t = ctx.ref(env, sd, K.START_INDICES[env], goal=K.RRT_GOALS[env])
        assert SC.entitled(t) and t.result == R.SUCCESS and t.goal_node > 0 and t.stats.rejected_edges >= 1
        check_tree(o["nodes"][env], int(o["n_nodes"][env]), t, "rrt env %d" % env)
        na = int(o["n_actions"][env])
        assert int(o["result"][env]) == R.SUCCESS and na == t.depth[t.goal_node] and int(o["halton_next"][env]) == t.halton_next
        np.testing.assert_allclose(o["plan"][env, :na], np.array(t.actions_to(t.goal_node)), atol=ATOL)


# ---------------------------------------------------------------- 3
def test_the_shrink_and_the_key_compared_with_the_number_of_landmarks(ctxb):
    c, sd, start = ctxb, SC.SHRINK_DISTANCE, SC.B_START_INDEX
    envs = [SC.B_NEAR, SC.B_KEY_HIGH, SC.B_PLAIN]
    want_sd = {}
    for env in envs:
        t = c.ref(env, sd, start, n_accept=SC.B_ACCEPT)
        assert SC.entitled(t) and t.result == R.SUCCESS
        want_sd[env] = t.sd
        c.sampler(env, SC.B_ACCEPT, sd)
        o = host(c.eng.em_plan(c.i32([env]), c.i32([start]), SC.CAP, 0, want_nodes=True))
        check_tree(o["nodes"][0], int(o["n_nodes"][0]), t, "em env %d" % env)
        assert int(o["halton_next"][0]) == t.halton_next and int(o["result"][0]) == R.SUCCESS
        assert check_pick(c, o, 0, env) == t.leaves()
    # NEAR: key 0 below the count, 0.04 m away -> optimize2's clamp to 0: the plain tree, nothing refused
    near = c.ref(SC.B_NEAR, sd, start, n_accept=SC.B_ACCEPT)
    assert want_sd[SC.B_NEAR] == 0.0 and near.stats.shrunk and near.halton_next == start + SC.B_ACCEPT
    # KEY_HIGH: within safe_distance of its nearest landmark, whose key is not below the count -> not shrunk, edges refused
    high = c.ref(SC.B_KEY_HIGH, sd, start, n_accept=SC.B_ACCEPT)
    keys, xy = c.lm[SC.B_KEY_HIGH]
    d = np.hypot(xy[:, 0] - c.root[SC.B_KEY_HIGH][0], xy[:, 1] - c.root[SC.B_KEY_HIGH][1])
    assert d.min() < sd and keys[int(np.argmin(d))] >= len(keys)
    assert want_sd[SC.B_KEY_HIGH] == sd and not high.stats.shrunk and high.stats.rejected_edges >= 1
    # PLAIN: shrunk to distance - 0.1
    assert 0.5 < want_sd[SC.B_PLAIN] < sd and c.ref(SC.B_PLAIN, sd, start, n_accept=SC.B_ACCEPT).stats.shrunk
    # rrt_planner, one call: NEAR goes below -1e-3 (the deviation: failure at once), KEY_HIGH keeps 3.0, PLAIN shrinks unclamped
    o = rrt(c, envs, SC.B_RRT_GOALS[envs], [start] * 3)
    assert c.eng.status() == 0
    for row, env in enumerate(envs):
        t = c.ref(env, sd, start, goal=SC.B_RRT_GOALS[env])
        assert SC.entitled(t)
        check_tree(o["nodes"][row], int(o["n_nodes"][row]), t, "rrt env %d" % env)
        assert int(o["result"][row]) == t.result and int(o["halton_next"][row]) == t.halton_next
        if env == SC.B_NEAR:
            assert t.sd < -1e-3 and t.result == R.SAMPLING_FAILURE
            check_failed(o, row, 1, start, "the deviation")
        else:
            assert t.result == R.SUCCESS and t.goal_node > 0 and int(o["n_actions"][row]) == t.depth[t.goal_node]
            assert t.sd == (sd if env == SC.B_KEY_HIGH else want_sd[env])


# ---------------------------------------------------------------- 4
def test_a_sampling_failure_is_a_result_and_leaves_the_other_trees_alone(ctxb):
    c, start = ctxb, SC.B_START_INDEX
    before = c.live_state()
    # (a) sampleNode: 1001 unsafe points.  KEY_HIGH is not shrunk at 60 m, PLAIN is
    sd = SC.FAIL_DISTANCE
    bad, good = c.ref(SC.B_KEY_HIGH, sd, start, n_accept=SC.B_ACCEPT), c.ref(SC.B_PLAIN, sd, start, n_accept=SC.B_ACCEPT)
    assert bad.result == R.SAMPLING_FAILURE and len(bad) == 1 and bad.stats.rejected_samples == 1001 and bad.stats.gate_margin > 1.0
    assert good.result == R.SUCCESS and SC.entitled(good)
    c.sampler(SC.B_PLAIN, SC.B_ACCEPT, sd)
    both = host(c.eng.em_plan(c.i32([SC.B_KEY_HIGH, SC.B_PLAIN]), c.i32([start, start]), SC.CAP, 0, want_nodes=True))
    alone = host(c.eng.em_plan(c.i32([SC.B_PLAIN]), c.i32([start]), SC.CAP, 0, want_nodes=True))
    assert c.eng.status() == 0
    check_failed(both, 0, 1, start + 1001, "sampleNode")
    np.testing.assert_allclose(both["nodes"][0, 0, :3], c.root[SC.B_KEY_HIGH], atol=ATOL)
    for k in alone:
        np.testing.assert_array_equal(both[k][1], alone[k][0], err_msg=k)
    check_tree(alone["nodes"][0], int(alone["n_nodes"][0]), good, "beside a failure")
    assert check_pick(c, alone, 0, SC.B_PLAIN) == good.leaves()
    # a call in which no tree has a leaf: nothing is scored
    none = host(c.eng.em_plan(c.i32([SC.B_KEY_HIGH]), c.i32([start]), SC.CAP, 0, want_nodes=True))
    check_failed(none, 0, 1, start + 1001, "no leaf in the call")
    assert c.eng.status() == 0
    o = rrt(c, [SC.B_KEY_HIGH, SC.B_PLAIN], SC.B_RRT_GOALS[[SC.B_KEY_HIGH, SC.B_PLAIN]], [start, start])
    check_failed(o, 0, 1, start + 1001, "rrt sampleNode")
    g = c.ref(SC.B_PLAIN, sd, start, goal=SC.B_RRT_GOALS[SC.B_PLAIN])
    assert SC.entitled(g) and g.result == R.SUCCESS
    check_tree(o["nodes"][1], int(o["n_nodes"][1]), g, "rrt beside a failure")
    assert int(o["n_actions"][1]) == g.depth[g.goal_node]
    # (b) the connect counter: every edge from WALLED's root is refused at 3.9 m - 1001 refusals in a row
    sd = SC.WALLED_DISTANCE
    bad, good = c.ref(SC.B_WALLED, sd, start, n_accept=SC.B_ACCEPT), c.ref(SC.B_PLAIN, sd, start, n_accept=SC.B_ACCEPT)
    assert bad.result == R.SAMPLING_FAILURE and len(bad) == 1 and bad.stats.rejected_edges == 1001 and SC.entitled(bad)
    assert bad.halton_next == start + 1001 + bad.stats.rejected_samples and good.result == R.SUCCESS and SC.entitled(good)
    c.sampler(SC.B_PLAIN, SC.B_ACCEPT, sd)
    both = host(c.eng.em_plan(c.i32([SC.B_PLAIN, SC.B_WALLED]), c.i32([start, start]), SC.CAP, 0, want_nodes=True))
    check_failed(both, 1, 1, bad.halton_next, "connect counter")
    check_tree(both["nodes"][0], int(both["n_nodes"][0]), good, "beside a connect failure")
    assert check_pick(c, both, 0, SC.B_PLAIN) == good.leaves()
    o = rrt(c, [SC.B_WALLED], SC.B_RRT_GOALS[[SC.B_WALLED]], [start])
    check_failed(o, 0, 1, bad.halton_next, "rrt connect counter")
    assert c.eng.status() == 0
    for x, y in zip(before, c.live_state()):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------- 5
def test_rrt_goal_edge_refused_is_success_with_an_empty_plan(ctx):
    sd = SC.SAFE_DISTANCE
    ctx.sampler(0, SC.N_ACCEPT, sd)
    o = rrt(ctx, list(range(K.N_ENVS)), SC.UNSAFE_GOALS, K.START_INDICES)
    assert ctx.eng.status() == 0
    for env in range(K.N_ENVS):
        t = ctx.ref(env, sd, K.START_INDICES[env], goal=SC.UNSAFE_GOALS[env])
        assert SC.entitled(t) and t.result == R.SUCCESS and t.goal_node == -1 and t.goal_edge_refused and 1 < len(t) < SC.CAP
        check_tree(o["nodes"][env], int(o["n_nodes"][env]), t, "refused goal env %d" % env)  # (n_nodes: the goal is not counted)
        assert int(o["result"][env]) == R.SUCCESS and int(o["n_actions"][env]) == 0 and np.all(o["plan"][env] == 0.0)
        assert int(o["halton_next"][env]) == t.halton_next
        last = o["nodes"][env][int(o["n_nodes"][env]) - 1]
        assert np.hypot(*(last[:2] - SC.UNSAFE_GOALS[env])) > 1e-3  # the goal is not in nodes_out


# ---------------------------------------------------------------- 6
def error_code(call):
    from drl_graph_exploration_amd._lib import DrlgxError
    with pytest.raises(DrlgxError) as ei:
        call()
    return int(str(ei.value).split("drlgx error ")[1].split(":")[0])


def test_refusals_with_the_opt_in_on(ctx):
    sel, starts = ctx.i32(list(range(K.N_ENVS))), ctx.i32(K.START_INDICES)
    goals = ctx.f64(K.RRT_GOALS)
    before = ctx.live_state()
    assert ctx.eng.sampler_obstacles is True
    ctx.eng.set_sampler_parameter(0.1, safe_distance=-0.5)
    assert error_code(lambda: ctx.eng.em_plan(sel, starts, SC.CAP)) == DRLGX_E_INVALID
    assert error_code(lambda: ctx.eng.rrt_plan(sel, sel, goals, starts, SC.CAP)) == DRLGX_E_INVALID
    ctx.eng.set_sampler_parameter(0.1, safe_distance=1.0, dubins_control_model_enabled=True)
    assert error_code(lambda: ctx.eng.em_plan(sel, starts, SC.CAP)) == DRLGX_E_INVALID
    assert error_code(lambda: ctx.eng.rrt_plan(sel, sel, goals, starts, SC.CAP)) == DRLGX_E_INVALID
    assert ctx.eng.status() == 0
    for x, y in zip(before, ctx.live_state()):
        assert x.tobytes() == y.tobytes()
    ctx.eng.set_sampler_parameter(0.1)


# ---------------------------------------------------------------- 7
def safe_ini(lo, max_nodes, planner_sd="1.0"):
    cp = ConfigParser()
    cp.read_dict({
        "Sensor Model": dict(bearing_noise="0.5", range_noise="0.02", min_bearing="-179.9", max_bearing="179.9", min_range="0.1", max_range="6.0"),
        "Control Model": dict(translation_noise="0.1", rotation_noise="0.2"),
        "Environment": dict(min_x="-6", max_x="6", min_y="-6", max_y="6", max_steps="5000", safe_distance="0.0"),
        "Virtual Map": dict(resolution="2.0", sigma0="1.0", num_samples="1"),
        "Simulator": dict(seed=str(lo), lo=str(lo), num=str(K.NUM_LANDMARKS), sigma_x0="0.05", sigma_y0="0.05", sigma_theta0="0.01"),
        "Planner": dict(seed=str(K.DEFAULT_SEED), angle_weight="0.4", distance_weight0="5.0", distance_weight1="2.0", d_weight="0.0",
                        max_edge_length="2.0", max_nodes=repr(max_nodes), occupancy_threshold="0.4", safe_distance=planner_sd,
                        algorithm="EM_AOPT", reg_out="false", dubins_control_model_enabled="false"),
    })
    return cp


def same_odoms(got, want):
    got, want = np.array(got).reshape(-1, 3), np.array(want).reshape(-1, 3)
    np.testing.assert_array_equal(got[:, :2], want[:, :2])
    np.testing.assert_allclose(got[:, 2], want[:, 2], rtol=0, atol=THETA_ATOL)


def test_facades_under_a_planner_safe_distance_of_one():
    from drl_graph_exploration_amd import planner2d
    from drl_graph_exploration_amd.pyplanner2d import EMExplorer
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    from staged_facade import StagedEMExplorer
    start = tuple(K.STARTS[0])
    h0 = planner2d.halton_start_index(K.DEFAULT_SEED)
    cap = planner2d.EMPlanner2D.MAX_TREE_NODES
    goal = (float(K.RRT_GOALS[0][0]), float(K.RRT_GOALS[0][1]))
    for make in (StagedEMExplorer, EMExplorer):
        ex = make(safe_ini(0, 0.2), start=start, **({"obstacle_logic": True} if make is EMExplorer else {}))
        for act in K.SCRIPT:
            ex.simulate(act)
        eng, dev = ex.engine, ex.engine.device
        if make is StagedEMExplorer:
            # the default still refuses; the opt-in is the planner's attribute
            with pytest.raises(NotImplementedError):
                ex._planner.optimize2(ex._slam, ex._virtual_map)
            planner = planner2d.EMPlanner2D(ex._planner_params, ex._sim.sensor_model, ex._sim.control_model, obstacle_logic=True)
            assert planner.obstacle_logic is True and planner2d.EMPlanner2D.obstacle_logic is False
            planner._parameter.dubins_control_model_enabled = True
            with pytest.raises(NotImplementedError):
                planner.optimize2(ex._slam, ex._virtual_map)
            planner._parameter.dubins_control_model_enabled = False
        else:
            planner = ex._planner
        sel, st = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([h0], dtype=torch.int32, device=dev)
        eng.set_sampler_obstacles(True)
        eng.set_sampler_parameter(0.2, safe_distance=1.0)
        want = host(eng.em_plan(sel, st, cap, 0))
        na = int(want["n_actions"][0])
        assert na >= 1 and int(want["n_nodes"][0]) > 3 and int(want["result"][0]) == R.SUCCESS
        if make is StagedEMExplorer:
            assert planner.optimize2(ex._slam, ex._virtual_map) == planner2d.OptimizationResult.SUCCESS
        else:
            assert ex.plan() is True
        got = [[e.get_odoms()[0].x, e.get_odoms()[0].y, e.get_odoms()[0].theta] for e in planner.iter_solution()]
        same_odoms(got, want["plan"][0, :na][::-1])
        assert planner.halton_next == int(want["halton_next"][0])
        st2 = torch.tensor([planner.halton_next], dtype=torch.int32, device=dev)
        far = torch.tensor([10 ** 6], dtype=torch.int32, device=dev)
        rw = host(eng.rrt_plan(sel, far, torch.tensor([goal], dtype=torch.float64, device=dev), st2, cap))
        if make is StagedEMExplorer:
            ok = planner.rrt_planner(ex._slam, ex._virtual_map, 10 ** 6, goal[0], goal[1]) == planner2d.OptimizationResult.SUCCESS
        else:
            ok = ex.rrt_plan(10 ** 6, goal)
        assert ok == (int(rw["result"][0]) == R.SUCCESS) and planner.halton_next == int(rw["halton_next"][0])
        path = []
        for edge in planner.iter_solution():
            path.insert(0, edge.get_odoms()[0])
        same_odoms([[p.x, p.y, p.theta] for p in path], rw["plan"][0, :int(rw["n_actions"][0])])
        eng.close()
    env = VecExplorationEnv(K.MAP, 2, env_index=0, test=True, starts=K.STARTS[:2], num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES,
                            n_rollouts=0)
    try:
        e = env.engine
        sel = torch.arange(2, dtype=torch.int32, device=env.device)
        st = torch.full((2,), h0, dtype=torch.int32, device=env.device)
        e.set_sampler_parameter(0.3, safe_distance=0.0)
        e.set_sampler_obstacles(True)
        e.set_sampler_parameter(0.08, safe_distance=1.0)
        want = host(e.em_plan(sel, st, 2048, int(env.cfg.algorithm)))
        gk = torch.full((2,), 10 ** 6, dtype=torch.int32, device=env.device)
        want_rrt = host(e.rrt_plan(sel, gk, torch.tensor(K.RRT_GOALS[:2], device=env.device), torch.tensor(want["halton_next"], device=env.device), 2048))
        e.set_sampler_obstacles(False)
        e.set_sampler_parameter(0.3, safe_distance=0.0)
        acts, n_act, result = env.em_plan(max_nodes=0.08, safe_distance=1.0)
        np.testing.assert_array_equal(acts.cpu().numpy(), want["plan"])
        np.testing.assert_array_equal(n_act.cpu().numpy(), want["n_actions"])
        np.testing.assert_array_equal(result.cpu().numpy(), want["result"])
        np.testing.assert_array_equal(env._halton_next.cpu().numpy(), want["halton_next"])
        assert e.sampler_parameter == (0.3, 0.0, False) and e.sampler_obstacles is False
        acts, n_act, result = env.rrt_plan(gk, torch.tensor(K.RRT_GOALS[:2], device=env.device), safe_distance=1.0)
        np.testing.assert_array_equal(acts.cpu().numpy(), want_rrt["plan"])
        np.testing.assert_array_equal(result.cpu().numpy(), want_rrt["result"])
        assert e.sampler_parameter == (0.3, 0.0, False) and e.sampler_obstacles is False
        # the engine itself is back at its refusal: a non-zero safe_distance without the opt-in
        e.set_sampler_parameter(0.08, safe_distance=1.0)
        assert error_code(lambda: e.em_plan(sel, st, 2048, int(env.cfg.algorithm))) == DRLGX_E_INVALID
    finally:
        env.close()
