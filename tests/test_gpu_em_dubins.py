"""GPU tests (run with -m gpu on an MI355X) of the tree sampler's Dubins control model - the kDubins instantiations of k_em_tree and
k_em_leaves_dubins (csrc/k_em_tree.hip) behind Engine.set_dubins_library - against tests/em_dubins_ref.py on the cases of
tests/em_dubins_cases.py.  As in tests/test_gpu_em_safe.py the restatement runs on the engine's own read-back belief (inputs, not
results), and the margins that entitle a case to exact comparisons - nearest-node, tolerance-radius, safety and isReached margins -
are asserted here again on that belief.

Exact: parents, library indices, step counts, n_nodes, halton_next, result, n_actions.  Node poses, distances and plan rows at the
project's pose tolerance, 1e-9 absolute.  The library read back from the engine: v, w, num_steps exact, end at
1e-15 absolute (the host build and numpy both go through the C library's cos / sin / atan2; the largest difference seen is printed).

A library's size is always even (two signs), so the size "65" of the 64-entry stride's far side does not exist: 66 stands for it."""
from configparser import ConfigParser

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_dubins_cases as DC  # noqa: E402
import em_dubins_ref as D  # noqa: E402
import em_tree_cases as K  # noqa: E402
import em_tree_ref as R  # noqa: E402

ATOL = 1e-9
DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3


class Ctx(object):
    """One engine, its beliefs read back once."""

    def __init__(self, max_actions=DC.MAX_ACTIONS):
        from drl_graph_exploration_amd import default_config
        from drl_graph_exploration_amd.engine import Engine
        self.n = DC.N_ENVS
        self.cfg = default_config(K.MAP, num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES, max_actions=max_actions)
        self.eng = Engine(self.cfg, self.n, 0)
        self.eng.set_dubins_library(DC.LIB_36)  # (without the feature every test of this file fails here)
        self.eng.reset(np.arange(self.n), np.array(DC.SEEDS), starts=np.array(DC.STARTS))
        for act in K.SCRIPT:
            self.eng.step(torch.tensor([act] * self.n, dtype=torch.float64, device=self.eng.device))
        assert self.eng.status() == 0
        self.dev = self.eng.device
        self.root = [self.eng.poses(i)[0][-1] for i in range(self.n)]
        self.lm = [self.eng.landmarks(i)[:2] for i in range(self.n)]
        self._trees = {}

    def i32(self, v):
        return torch.tensor(v, dtype=torch.int32, device=self.dev)

    def f64(self, v):
        return torch.tensor(np.asarray(v, dtype=np.float64), device=self.dev)

    def ref(self, name, env, start, goal, sd=0.0, cap=DC.CAP):
        key = (name, env, start, tuple(goal), sd, cap)
        if key not in self._trees:
            keys, xy = self.lm[env]
            self._trees[key] = DC.tree_of(self.cfg, self.root[env], DC.library(name), start, goal, keys, xy, sd, cap)
        return self._trees[key]

    def use(self, params, sd=0.0, dubins=True):
        self.eng.set_dubins_library(params)
        self.eng.set_sampler_obstacles(sd != 0.0)
        self.eng.set_sampler_parameter(0.1, safe_distance=sd, dubins_control_model_enabled=dubins)

    def rrt(self, sel, goals, starts, cap=DC.CAP):
        none = self.i32([10 ** 6] * len(sel))  # (beyond key_size: the point is the goal)
        o = self.eng.rrt_plan(self.i32(sel), none, self.f64(goals), self.i32(starts), cap, want_nodes=True)
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}

    def live_state(self):
        out = []
        for i in range(self.n):
            out += [self.eng.poses(i)[0], self.eng.poses(i)[1], self.eng.landmarks(i)[1], *self.eng.virtual_map(i)[:3]]
        return [np.array(a, copy=True) for a in out] + [self.eng.counts_dev().cpu().numpy()]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.eng.close()


def error_code(call):
    from drl_graph_exploration_amd._lib import DrlgxError
    with pytest.raises(DrlgxError) as ei:
        call()
    return int(str(ei.value).split("drlgx error ")[1].split(":")[0])


def check_tree(o, row, t, tag):
    """Parents, library indices, step counts, n_nodes, halton_next, result, n_actions exact; poses, distances, plan rows at 1e-9."""
    n_nodes = int(o["n_nodes"][row])
    assert n_nodes == len(t), tag
    nd = o["nodes"][row][:n_nodes]
    np.testing.assert_array_equal(nd[:, 3].astype(np.int64), np.array(t.parent), err_msg=tag)
    np.testing.assert_array_equal(nd[:, 5:8], np.array(t.action), err_msg=tag)  # library index, num_steps, 0
    xyt = t.xytheta()
    dth = np.abs(np.arctan2(np.sin(nd[:, 2] - xyt[:, 2]), np.cos(nd[:, 2] - xyt[:, 2])))
    dev = max(np.abs(nd[:, :2] - xyt[:, :2]).max(), dth.max(), np.abs(nd[:, 4] - np.array(t.distance)).max())
    assert dev <= ATOL, "%s: %.3e" % (tag, dev)
    assert int(o["result"][row]) == t.result and int(o["halton_next"][row]) == t.halton_next, tag
    rows = D.plan_rows(t)
    na = int(o["n_actions"][row])
    assert na == len(rows) == (t.depth[t.goal_node] if t.goal_node > 0 else 0), tag
    if na:
        got, want = o["plan"][row, :na], np.array(rows)
        dth = np.abs(np.arctan2(np.sin(got[:, 2] - want[:, 2]), np.cos(got[:, 2] - want[:, 2])))
        dev = max(dev, np.abs(got[:, :2] - want[:, :2]).max(), dth.max())
        assert dev <= ATOL, "%s plan: %.3e" % (tag, dev)
    assert np.all(o["plan"][row, na:] == 0.0), tag
    return dev


# ---------------------------------------------------------------- 1
def test_the_library_read_back_matches_the_restatement(ctx):
    from drl_graph_exploration_amd._lib import DrlgxError
    for name, p in list(DC.LIBS.items()) + [("shipped", DC.LIB_SHIPPED)]:
        assert ctx.eng.set_dubins_library(p) == (DC.SIZES.get(name) or DC.SHIPPED_SIZE)
        got, want = ctx.eng.dubins_library(), D.Library(p) if name == "shipped" else DC.library(name)
        np.testing.assert_array_equal(got["v"], want.v)
        np.testing.assert_array_equal(got["w"], want.w)
        np.testing.assert_array_equal(np.signbit(got["w"]), np.signbit(want.w))
        np.testing.assert_array_equal(got["num_steps"], want.num_steps)
        dev = np.abs(got["end"] - want.end).max()
        print("library %s: %d entries, end differs by at most %.3e" % (name, len(want), dev))
        assert dev <= 1e-15, name
    for bad in (dict(max_w=0.0), dict(dw=0.0), dict(dv=-0.1), dict(dt=0.0), dict(tolerance_radius=0.0), dict(max_v=0.4)):
        p = D.Params(*DC.LIB_36.values(), **bad)
        assert error_code(lambda: ctx.eng.set_dubins_library(p)) == DRLGX_E_INVALID, bad
    too_many = D.Params(*DC.LIB_SHIPPED.values(), dw=0.005)  # twice the shipped section's rates: 155 000 entries
    assert error_code(lambda: ctx.eng.set_dubins_library(too_many)) == DRLGX_E_CAPACITY
    assert ctx.eng.dubins_library_size() == DC.SHIPPED_SIZE  # (a refused library leaves the loaded one)
    assert ctx.eng.set_dubins_library(None) == 0 and len(ctx.eng.dubins_library()["v"]) == 0


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["36", "64", "66", "320"])
def test_trees_match_the_restatement(ctx, name):
    ctx.use(DC.LIBS[name])
    envs = list(range(DC.N_ENVS))
    o = ctx.rrt(envs, DC.GOALS[name], DC.START_INDICES)
    assert ctx.eng.status() == 0
    reached, winners, same, other = 0, set(), 0, 0
    for env in envs:
        t = ctx.ref(name, env, DC.START_INDICES[env], DC.GOALS[name][env])
        st = t.stats
        assert DC.entitled(t), (env, min(t.margin), st.gate_margin, st.match_margin)
        dev = check_tree(o, env, t, "library %s env %d" % (name, env))
        reached += t.result == R.SUCCESS and t.goal_node > 0 and len(t) - 1 >= 8 and st.rejected_edges >= 1
        winners |= set(st.winners)
        same += st.multi_same_stride
        other += st.multi_other_stride
        print("library %s env %d: %d nodes, %d points drawn, %d connects without a path, %d steps, margins %.1e / %.1e / %.1e, worst %.1e" % (
            name, env, len(t), st.drawn, st.no_match, int(o["n_actions"][env]), min(t.margin), st.match_margin, st.gate_margin, dev))
    assert reached >= 3 and 0 in winners and same >= 1
    if name == "320":  # the stride's edges, the last entry, matches in two strides: the lowest index wins
        assert {0, 63, 64, 319} <= winners and other >= 1
    # the exact pre-filter changes nothing: the same call with every scan made
    ctx.eng.set_dubins_prefilter(False)
    try:
        full = ctx.rrt(envs, DC.GOALS[name], DC.START_INDICES)
    finally:
        ctx.eng.set_dubins_prefilter(True)
    for k in o:
        np.testing.assert_array_equal(o[k], full[k], err_msg=k)


# ---------------------------------------------------------------- 3
def test_unsafe_intermediate_poses_refuse_and_the_end_poses_are_not_tested(ctx):
    ctx.use(DC.LIB_320, sd=DC.SAFE_DISTANCE)
    try:
        sel = [c[0] for c in DC.OBSTACLE_CASES]
        o = ctx.rrt(sel, [c[1] for c in DC.OBSTACLE_CASES], [c[2] for c in DC.OBSTACLE_CASES])
        assert ctx.eng.status() == 0
        unsafe = first = last = reached = 0
        for row, (env, goal, start) in enumerate(DC.OBSTACLE_CASES):
            t = ctx.ref("320", env, start, goal, sd=DC.SAFE_DISTANCE)
            st = t.stats
            assert DC.entitled(t) and st.rejected_samples >= 1, (row, min(t.margin), st.gate_margin, st.match_margin)
            check_tree(o, row, t, "obstacles case %d" % row)
            unsafe, first, last = unsafe + st.unsafe_path, first + st.unsafe_first_accepted, last + st.unsafe_last_accepted
            reached += t.goal_node > 0
        assert unsafe >= 4 and first >= 1 and last >= 1 and reached >= 2
    finally:
        ctx.eng.set_sampler_obstacles(False)


# ---------------------------------------------------------------- 4
def test_the_connect_counter_ends_a_tree_and_a_goal_edge_without_a_path_is_an_empty_plan(ctx):
    before = ctx.live_state()
    ctx.use(DC.LIB_TIGHT)
    o = ctx.rrt([0, 1], DC.GOALS["36"][:2], [5, 5])
    for row in range(2):
        assert int(o["result"][row]) == R.SAMPLING_FAILURE and int(o["n_nodes"][row]) == 1 and int(o["halton_next"][row]) == 5 + 1001
        assert int(o["n_actions"][row]) == 0 and np.all(o["plan"][row] == 0.0)
    ctx.use(DC.LIB_320)
    envs = list(range(DC.N_ENVS))
    o = ctx.rrt(envs, DC.REFUSED_GOALS, DC.START_INDICES)
    for env in envs:
        t = ctx.ref("320", env, DC.START_INDICES[env], DC.REFUSED_GOALS[env])
        assert DC.entitled(t) and t.result == R.SUCCESS and t.goal_edge_refused and t.goal_node == -1 and 1 < len(t) < DC.CAP
        check_tree(o, env, t, "refused goal env %d" % env)  # (n_nodes: the goal is not counted; n_actions 0)
    assert ctx.eng.status() == 0
    for x, y in zip(before, ctx.live_state()):
        np.testing.assert_array_equal(x, y)


# (library, environment, nodes): cases of test_trees_match_the_restatement whose tree reaches its goal, with the tree's size, the goal
# node included - at least one per library, the smallest there are (the 64- and 320-entry libraries have none below 92 and 74)
LAST_SLOT_CASES = [("36", 0, 10), ("36", 1, 24), ("64", 2, 92), ("66", 0, 21), ("66", 2, 18), ("320", 0, 74)]


@pytest.mark.parametrize("name, env, size", LAST_SLOT_CASES)
def test_a_goal_reached_by_the_node_that_fills_the_table_is_not_connected(ctx, name, env, size):
    """A table one node short of the whole tree: the node that reaches the goal takes the last slot, the goal edge is not made -
    SAMPLING_FAILURE, no plan, and everything up to there as with the full table."""
    ctx.use(DC.LIBS[name])
    start, goal, tag = DC.START_INDICES[env], DC.GOALS[name][env], "library %s env %d" % (name, env)
    t = ctx.ref(name, env, start, goal)
    assert DC.entitled(t) and len(t) == size and t.goal_node == size - 1, tag
    whole = ctx.rrt([env], [goal], [start])
    o = ctx.rrt([env], [goal], [start], cap=size - 1)
    assert ctx.eng.status() == 0
    assert int(whole["n_nodes"][0]) == size and int(whole["result"][0]) == R.SUCCESS, tag
    assert int(o["result"][0]) == R.SAMPLING_FAILURE and int(o["n_nodes"][0]) == size - 1, tag
    assert int(o["n_actions"][0]) == 0 and np.all(o["plan"][0] == 0.0), tag
    assert int(o["halton_next"][0]) == int(whole["halton_next"][0]), tag
    np.testing.assert_array_equal(o["nodes"][0][:size - 1], whole["nodes"][0][:size - 1], err_msg=tag)
    short = ctx.ref(name, env, start, goal, cap=size - 1)
    assert DC.entitled(short) and short.result == R.SAMPLING_FAILURE and len(short) == size - 1 and short.goal_node == -1, tag
    check_tree(o, 0, short, tag)


# ---------------------------------------------------------------- 5
def test_refusals(ctx):
    sel, starts = ctx.i32(list(range(DC.N_ENVS))), ctx.i32(DC.START_INDICES)
    goals, none = ctx.f64(DC.GOALS["320"]), ctx.i32([10 ** 6] * DC.N_ENVS)
    before = ctx.live_state()
    ctx.use(DC.LIB_320)
    # optimize2 under the Dubins model stays refused
    assert error_code(lambda: ctx.eng.em_plan(sel, starts, DC.CAP)) == DRLGX_E_INVALID
    # a non-zero safe_distance without the obstacle opt-in, a negative one with it
    ctx.eng.set_sampler_parameter(0.1, safe_distance=1.0, dubins_control_model_enabled=True)
    assert error_code(lambda: ctx.eng.rrt_plan(sel, none, goals, starts, DC.CAP)) == DRLGX_E_INVALID
    # the library cleared: the flag is refused as before, the plain model is served
    ctx.eng.set_dubins_library(None)
    ctx.eng.set_sampler_parameter(0.1, dubins_control_model_enabled=True)
    assert error_code(lambda: ctx.eng.rrt_plan(sel, none, goals, starts, DC.CAP)) == DRLGX_E_INVALID
    assert error_code(lambda: ctx.eng.em_plan(sel, starts, DC.CAP)) == DRLGX_E_INVALID
    ctx.eng.set_sampler_parameter(0.1)
    plain = ctx.eng.rrt_plan(sel, none, goals, starts, DC.CAP, want_nodes=True)
    assert int(plain["n_nodes"].min()) > 1 and float(plain["nodes"][0, 1, 5:8].abs().sum()) > 0  # (an edge odometry, not an index)
    assert ctx.eng.status() == 0
    for x, y in zip(before, ctx.live_state()):
        assert x.tobytes() == y.tobytes()


def test_a_path_of_more_steps_than_max_actions_refuses_the_call():
    """36 entries, env 0: 12 steps - served at max_actions = 12; 320 entries, env 0: 36 steps - DRLGX_E_CAPACITY."""
    c = Ctx(max_actions=12)
    try:
        t = c.ref("36", 0, DC.START_INDICES[0], DC.GOALS["36"][0])
        assert DC.entitled(t) and t.depth[t.goal_node] == 12
        c.use(DC.LIB_36)
        check_tree(c.rrt([0], [DC.GOALS["36"][0]], [DC.START_INDICES[0]]), 0, t, "exactly max_actions")
        t = c.ref("320", 0, DC.START_INDICES[0], DC.GOALS["320"][0])
        assert DC.entitled(t) and t.depth[t.goal_node] > 12
        c.use(DC.LIB_320)
        before = c.live_state()
        assert error_code(lambda: c.rrt([0], [DC.GOALS["320"][0]], [DC.START_INDICES[0]])) == DRLGX_E_CAPACITY
        assert c.eng.status() == 0
        for x, y in zip(before, c.live_state()):
            assert x.tobytes() == y.tobytes()
    finally:
        c.eng.close()


# ---------------------------------------------------------------- 6
def dubins_ini(lo, p):
    cp = ConfigParser()
    cp.read_dict({
        "Sensor Model": dict(bearing_noise="0.5", range_noise="0.02", min_bearing="-179.9", max_bearing="179.9", min_range="0.1", max_range="6.0"),
        "Control Model": dict(translation_noise="0.1", rotation_noise="0.2"),
        "Environment": dict(min_x="-6", max_x="6", min_y="-6", max_y="6", max_steps="5000", safe_distance="0.0"),
        "Virtual Map": dict(resolution="2.0", sigma0="1.0", num_samples="1"),
        "Simulator": dict(seed=str(lo), lo=str(lo), num=str(K.NUM_LANDMARKS), sigma_x0="0.05", sigma_y0="0.05", sigma_theta0="0.01"),
        "Planner": dict(seed=str(K.DEFAULT_SEED), angle_weight="0.4", distance_weight0="5.0", distance_weight1="2.0", d_weight="0.0",
                        max_edge_length="2.0", max_nodes="0.2", occupancy_threshold="0.4", safe_distance="0.0", algorithm="EM_AOPT",
                        reg_out="false", dubins_control_model_enabled="true"),
        "Dubins": dict(zip(D.FIELDS, [repr(x) for x in p.values()])),
    })
    return cp


def test_facades_against_the_engine_call():
    from drl_graph_exploration_amd import planner2d
    from drl_graph_exploration_amd.pyplanner2d import EMExplorer
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    from staged_facade import StagedEMExplorer
    h0 = planner2d.halton_start_index(K.DEFAULT_SEED)
    cap = planner2d.EMPlanner2D.MAX_TREE_NODES
    goal = tuple(DC.FACADE_GOALS[0])
    for make in (StagedEMExplorer, EMExplorer):
        ex = make(dubins_ini(0, DC.LIB_320), start=tuple(DC.STARTS[0]), **({"dubins_paths": True} if make is EMExplorer else {}))
        for act in K.SCRIPT:
            ex.simulate(act)
        eng, dev = ex.engine, ex.engine.device
        if make is StagedEMExplorer:
            with pytest.raises(NotImplementedError):  # the flag alone still raises
                ex._planner.rrt_planner(ex._slam, ex._virtual_map, 10 ** 6, goal[0], goal[1])
            planner = planner2d.EMPlanner2D(ex._planner_params, ex._sim.sensor_model, ex._sim.control_model, dubins_paths=True)
            with pytest.raises(NotImplementedError):
                planner.optimize2(ex._slam, ex._virtual_map)
        else:
            planner = ex._planner
            with pytest.raises(NotImplementedError):
                ex.plan()
        lib = list(planner.iter_dubins_library())
        want_lib = DC.library("320")
        assert len(lib) == 320 and planner.get_dubins_path(319).num_steps == want_lib.num_steps[319]
        assert [d.v for d in lib] == list(want_lib.v) and abs(lib[7].end.x - want_lib.end[7, 0]) <= 1e-15
        sel, st = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([h0], dtype=torch.int32, device=dev)
        far = torch.tensor([10 ** 6], dtype=torch.int32, device=dev)
        eng.set_sampler_parameter(0.2, dubins_control_model_enabled=True)
        want = eng.rrt_plan(sel, far, torch.tensor([goal], dtype=torch.float64, device=dev), st, cap, want_nodes=True)
        want = {k: v.cpu().numpy() for k, v in want.items()}
        na = int(want["n_actions"][0])
        if make is StagedEMExplorer:
            ok = planner.rrt_planner(ex._slam, ex._virtual_map, 10 ** 6, goal[0], goal[1]) == planner2d.OptimizationResult.SUCCESS
        else:
            ok = ex.rrt_plan(10 ** 6, goal)
        assert ok == (int(want["result"][0]) == R.SUCCESS) and planner.halton_next == int(want["halton_next"][0]) and na >= 1
        odoms, steps, keys = [], [], []
        for edge in planner.iter_solution():  # leaf first
            odoms = [[p.x, p.y, p.theta] for p in edge.get_odoms()] + odoms
            steps.insert(0, len(edge.second.poses))
            keys.insert(0, (edge.first.key, edge.second.key))
            assert len(edge.get_odoms()) == len(edge.second.poses)
            last = edge.second.poses[-1]
            assert abs(last.x - edge.second.state.pose.x) <= ATOL and abs(last.y - edge.second.state.pose.y) <= ATOL
        np.testing.assert_array_equal(np.array(odoms)[:, :2], want["plan"][0, :na, :2])
        np.testing.assert_allclose(np.array(odoms)[:, 2], want["plan"][0, :na, 2], rtol=0, atol=1e-15)  # (Pose2 holds cos, sin)
        assert sum(steps) == na and all(b - a == s for (a, b), s in zip(keys, steps))
        eng.close()
    env = VecExplorationEnv(K.MAP, 2, env_index=0, test=True, starts=DC.STARTS[:2], num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES,
                            n_rollouts=0)
    try:
        e = env.engine
        sel = torch.arange(2, dtype=torch.int32, device=env.device)
        st = torch.full((2,), h0, dtype=torch.int32, device=env.device)
        gk = torch.full((2,), 10 ** 6, dtype=torch.int32, device=env.device)
        goals = torch.tensor(DC.FACADE_GOALS, dtype=torch.float64, device=env.device)
        par = planner2d.DubinsParameter()
        for f, v in zip(D.FIELDS, DC.LIB_320.values()):
            setattr(par, f, v)
        e.set_dubins_library(par)
        e.set_sampler_parameter(0.3, dubins_control_model_enabled=True)
        want = {k: v.cpu().numpy() for k, v in e.rrt_plan(sel, gk, goals, st, 2048).items() if v is not None}
        e.set_sampler_parameter(0.3)
        e.set_dubins_library(None)
        acts, n_act, result = env.rrt_plan(gk, goals, dubins=par)
        np.testing.assert_array_equal(acts.cpu().numpy(), want["plan"])
        np.testing.assert_array_equal(n_act.cpu().numpy(), want["n_actions"])
        np.testing.assert_array_equal(result.cpu().numpy(), want["result"])
        np.testing.assert_array_equal(env._halton_next.cpu().numpy(), want["halton_next"])
        assert int(want["n_actions"].max()) >= 1 and e.sampler_parameter  # (this env's own beliefs: one of the two goals is reached) == (0.3, 0.0, False)
    finally:
        env.close()
