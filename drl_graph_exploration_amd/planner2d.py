"""`planner2d` — the module surface of the reference's second pybind module (src/Planner2D.cpp:9-106) that the DRL
scripts use: the parameter classes and enums, and `EMPlanner2D(parameter, sensor_model, control_model)` with
`calculate_utility` / `line_planner` / `simulations_reward` over the engine of the simulation the models belong to
(`ss2d.Simulator2D`), and the tree sampler of the planners: `optimize2`, `rrt_planner`, `iter_solution`
(`drlgx_em_plan` / `drlgx_rrt_plan`) for the non-Dubins control model and, behind the opt-in `dubins_paths`, `rrt_planner` with
the Dubins control model (`get_dubins_path`, `iter_dubins_library`).  `optimize` and `iter_rrt` are outside the accelerated path
(SURVEY.md §8 "out of scope")."""
import enum
import math


def _mt19937_canonical(seed):
    """The first `std::generate_canonical<double, 53>` of `std::mt19937(seed)`: the single-integer seeding, one twist, two tempered
    32-bit outputs (the first is the low part) over 2^64."""
    mt = [0] * 624
    mt[0] = seed & 0xFFFFFFFF
    for i in range(1, 624):
        mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
    for i in range(624):
        y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
        mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)

    def temper(y):
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        return (y ^ (y >> 18)) & 0xFFFFFFFF

    u = (float(temper(mt[0])) + float(temper(mt[1])) * 4294967296.0) / 18446744073709551616.0
    return u if u < 1.0 else math.nextafter(1.0, 0.0)


def halton_start_index(seed):
    """The Halton index the planner's constructor starts from: `qrng_.setCount(rng_.uniformInt(0, 100000))` with `rng_(seed)`
    (Planner2D.cpp:36-45, RNG.h:64-77): floor(100001 u), clamped to [0, 100000]."""
    return min(max(int(math.floor(100001.0 * _mt19937_canonical(int(seed)))), 0), 100000)


class OptimizationAlgorithm(enum.IntEnum):
    """EMPlanner2D::OptimizationAlgorithm (include/em_exploration/Planner2D.h)."""
    EM_AOPT = 0
    EM_DOPT = 1
    OG_SHANNON = 2
    SLAM_OG_SHANNON = 3


class OptimizationResult(enum.IntEnum):
    SAMPLING_FAILURE = 0
    NO_SOLUTION = 1
    TERMINATION = 2
    SUCCESS = 3


class EMPlannerParameter(object):
    """EMPlanner2D::Parameter: the fields pyplanner2d.read_planner_params fills (scripts/envs/pyplanner2d.py:24-54)."""

    def __init__(self):
        self.verbose = False
        self.seed = 0
        self.max_edge_length = 2.0
        self.num_actions = 500
        self.max_nodes = 0.5
        self.angle_weight = 0.4
        self.distance_weight0 = 5.0
        self.distance_weight1 = 2.0
        self.d_weight = 0.0
        self.occupancy_threshold = 0.4
        self.safe_distance = 1.0
        self.alpha = 0.5
        self.reg_out = False
        self.algorithm = OptimizationAlgorithm.EM_AOPT
        self.dubins_control_model_enabled = False

        self.dubins_parameter = None

    def pprint(self):
        print("EMPlanner Parameters", vars(self))


class DubinsParameter(object):
    """EMPlanner2D::DubinsParameter (src/Planner2D.cpp:12-22): what Engine.set_dubins_library builds the path library from."""

    def __init__(self):
        self.max_w = self.dw = self.min_v = self.max_v = self.dv = self.dt = 0.0
        self.min_duration = self.max_duration = self.tolerance_radius = 0.0


class Dubins(object):
    """EMPlanner2D::Dubins as the binding shows it (src/Planner2D.cpp:24-29): one library path - v, w, end (Pose2), num_steps."""

    def __init__(self, v, w, end, num_steps):
        self.v, self.w, self.end, self.num_steps = float(v), float(w), end, int(num_steps)


class EMPlanner2D(object):
    """`EMPlanner2D(parameter, sensor_model, control_model)` (src/Planner2D.cpp:73-91) over the engine that the models'
    simulation owns: the calls the DRL scripts make - `calculate_utility` (static), `line_planner`, `simulations_reward` -
    run `drlgx_utility` / `drlgx_line_plan` / `drlgx_lookahead`; `leaf_cost` is the leaf evaluation of `optimize2`
    (`drlgx_em_cost`) for an action list the caller supplies, `leaf_entropy` the OG-Shannon cost of one (`drlgx_og_cost`), `leaf_slam_entropy` its SLAM-OG-Shannon cost (`drlgx_slam_og_cost`); `optimize2` and `rrt_planner` grow the sampler's tree on the device
    (`drlgx_em_plan` / `drlgx_rrt_plan`: non-Dubins control model, safe_distance 0 - or, with the attribute `obstacle_logic` set,
    any safe_distance >= 0 with the reference's isSafe / retry / shrink logic; it is an opt-in because the default refusal is what
    existing callers and tests rely on) and `iter_solution` walks the best path as the reference binding does.  The Halton index starts where the reference's constructor starts it and carries on from call to
    call.  With the attribute `dubins_paths` set (an opt-in for the same reason) and `dubins_control_model_enabled`, `set_parameter`
    loads `parameter.dubins_parameter` as the engine's Dubins library and `rrt_planner` runs the Dubins control model: an edge's
    `get_odoms()` is then one odometry per step, a node's `poses` the step poses; `get_dubins_path(i)` / `iter_dubins_library()`
    read the library; `optimize2` raises - unless the attribute `dubins_leaf_scoring` is set as well (an opt-in again:
    Engine.set_dubins_leaf_scoring): `optimize2` then grows the Dubins tree and scores every leaf with its non-core steps, and
    `iter_solution` yields the best leaf's edges, one odometry per step.  `optimize` and `iter_rrt` are outside the accelerated path."""
    MAX_TREE_NODES = 2048  # the node capacity of one tree (the engine's maximum)
    OptimizationAlgorithm = OptimizationAlgorithm
    OptimizationResult = OptimizationResult
    obstacle_logic = False  # True: the sampler's obstacle logic (Engine.set_sampler_obstacles) - a non-zero safe_distance is served
    dubins_paths = False    # True: the Dubins control model (Engine.set_dubins_library) - rrt_planner serves dubins_control_model_enabled
    dubins_leaf_scoring = False  # True (with dubins_paths): optimize2 serves it too (Engine.set_dubins_leaf_scoring)

    def __init__(self, parameter, sensor_model, control_model, obstacle_logic=False, dubins_paths=False, dubins_leaf_scoring=False):
        if obstacle_logic:
            self.obstacle_logic = True
        if dubins_paths:
            self.dubins_paths = True
        if dubins_leaf_scoring:
            self.dubins_leaf_scoring = True
        self._ses = sensor_model._session
        if self._ses is None or control_model._session is not self._ses:
            raise ValueError("the sensor and control models must come from one Simulator2D")
        self.set_parameter(parameter)
        self.halton_next = halton_start_index(parameter.seed)
        self._solution = []

    def get_parameter(self):
        return self._parameter

    def set_parameter(self, parameter):
        self._parameter = parameter
        self._ses.planner_params = parameter
        if self._ses.engine is not None:  # (constructed after SLAM2D.add_prior, as pyplanner2d.EMExplorer does)
            self._ses.engine.set_planner_parameter(parameter.angle_weight, parameter.distance_weight0, parameter.distance_weight1,
                                                   parameter.occupancy_threshold, parameter.max_edge_length, int(parameter.algorithm))
            self._ses.engine.set_sampler_parameter(parameter.max_nodes, parameter.safe_distance, parameter.dubins_control_model_enabled)
            self._ses.engine.set_sampler_obstacles(self.obstacle_logic)
            self._ses.engine.set_dubins_leaf_scoring(self.dubins_paths and self.dubins_leaf_scoring)
            if self.dubins_paths and parameter.dubins_control_model_enabled:
                load_dubins_library(self._ses.engine, parameter.dubins_parameter)

    @staticmethod
    def calculate_utility(virtual_map, distance, parameter):
        """EMPlanner2D::calculateUtility (Planner2D.cpp:354-366)."""
        import torch
        e = virtual_map._ses.require_engine()
        c = e.cfg
        if (parameter.distance_weight0, parameter.distance_weight1, parameter.occupancy_threshold) != \
                (c.distance_weight0, c.distance_weight1, c.occupancy_threshold):
            e.set_planner_parameter(parameter.angle_weight, parameter.distance_weight0, parameter.distance_weight1,
                                    parameter.occupancy_threshold, parameter.max_edge_length, int(parameter.algorithm))
        return float(e.utility(torch.tensor([float(distance)], dtype=torch.float64, device=e.device))[0])

    def line_planner(self, slam, virtual_map, n_key, fron_0, fron_1):
        """EMPlanner2D::line_planner (Planner2D.cpp:937-1041): goal = node `n_key` of the pose graph if it is one, else the
        frontier point (fron_0, fron_1); returns the list of Pose2 odometry actions."""
        import torch
        from . import ss2d
        e = self._ses.require_engine()
        if n_key < slam.key_size():
            fron_0, fron_1 = slam.get_key_points(n_key)
        ce = torch.zeros(1, dtype=torch.int32, device=e.device)
        goal = torch.tensor([[fron_0, fron_1]], dtype=torch.float64, device=e.device)
        acts, n = e.line_plan(ce, goal)
        e.check_status()
        return [ss2d.Pose2(*a) for a in acts[0, :int(n[0])].cpu().numpy()]

    def simulations_reward(self, slam, virtual_map, simulator, actions):
        """EMPlanner2D::simulations_reward (Planner2D.cpp:1416-1468): look-ahead with copies of the SLAM, map and
        simulator state (including its RNG streams); the live objects are not modified."""
        import torch
        e = self._ses.require_engine()
        A = e.cfg.max_actions
        if len(actions) > A:
            raise ValueError("plan longer than the engine's max_actions")
        acts = torch.zeros(1, A, 3, dtype=torch.float64)
        for k, a in enumerate(actions):
            acts[0, k] = torch.tensor([a.x, a.y, a.theta] if hasattr(a, "x") else list(a), dtype=torch.float64)
        n = torch.tensor([len(actions)], dtype=torch.int32, device=e.device)
        ce = torch.zeros(1, dtype=torch.int32, device=e.device)
        r = float(e.lookahead(ce, acts.to(e.device), n)[0])
        e.check_status()
        return r

    def leaf_cost(self, slam, virtual_map, actions, return_uncertainty=False):
        """The leaf evaluation of EMPlanner2D::optimize2 (Planner2D.cpp:1095-1104) for ONE action list of the wrapped
        simulation: updateTrajectory_EM (the FastMarginals2 covariance update, no re-solve), VirtualMap::updateInformation on a
        copy of the root's virtual map, node->uncertainty = calculateUncertainty_EM, node->cost = costFunction - the expected cost
        of the plan with the parameter's algorithm, without simulating it and without noise (`drlgx_em_cost`).  The live
        objects are not modified.  The sampler that builds optimize2's tree stays out of scope: `optimize2` itself raises."""
        e, ce, acts, n = self._one_candidate(actions)
        unc, cost = e.em_cost(ce, acts, n, int(self._parameter.algorithm))
        e.check_status()
        return (float(cost[0]), float(unc[0])) if return_uncertainty else float(cost[0])

    def leaf_entropy(self, slam, virtual_map, actions, return_cost=False):
        """calculateUncertainty_OG_SHANNON (Planner2D.cpp:368-392) for ONE action list of the wrapped simulation: the Shannon
        entropy of the occupancy map after the estimated landmarks, the trajectory and the plan's noise-free predicted poses have
        swept it (`drlgx_og_cost`); with `return_cost` also costFunction = entropy + distance * distance_weight.  No covariance,
        no simulation; the live objects are not modified.  `optimize2` under OptimizationAlgorithm.OG_SHANNON scores the leaves
        of its tree with this cost (`drlgx_og_plan`)."""
        e, ce, acts, n = self._one_candidate(actions)
        ent, cost = e.og_cost(ce, acts, n)
        e.check_status()
        return (float(ent[0]), float(cost[0])) if return_cost else float(ent[0])

    def leaf_slam_entropy(self, slam, virtual_map, actions, return_cost=False):
        """calculateUncertainty_SLAM_OG_SHANNON (Planner2D.cpp:394-416) for ONE action list of the wrapped simulation:
        w2 * (the entropy of `leaf_entropy`) + w1 * sum_l sqrt(det cov_l) over the landmarks after the plan's noise-free odometry
        and predicted measurements have updated their marginals (`drlgx_slam_og_cost`), with the root's weights w1 = alpha / (the
        same sum now), w2 = (1 - alpha) / (the entropy of the live map) and the parameter's `alpha`; with `return_cost` also
        costFunction = uncertainty + distance * distance_weight.  No simulation, no re-solve; the live objects are not modified.
        `optimize2` under OptimizationAlgorithm.SLAM_OG_SHANNON scores the leaves of its tree with this cost (`drlgx_og_plan`)."""
        e, ce, acts, n = self._one_candidate(actions)
        unc, cost = e.slam_og_cost(ce, acts, n, self._parameter.alpha)
        e.check_status()
        return (float(unc[0]), float(cost[0])) if return_cost else float(unc[0])

    def _one_candidate(self, actions):
        """(engine, cand_env, actions, n_actions) of one action list (Pose2 or (x, y, theta) entries) in the candidate layout."""
        import torch
        e = self._ses.require_engine()
        A = e.cfg.max_actions
        if len(actions) > A:
            raise ValueError("plan longer than the engine's max_actions")
        acts = torch.zeros(1, A, 3, dtype=torch.float64)
        for k, a in enumerate(actions):
            acts[0, k] = torch.tensor([a.x, a.y, a.theta] if hasattr(a, "x") else list(a), dtype=torch.float64)
        n = torch.tensor([len(actions)], dtype=torch.int32, device=e.device)
        ce = torch.zeros(1, dtype=torch.int32, device=e.device)
        return e, ce, acts.to(e.device), n

    def _tree_call(self, run, rrt=False):
        """One sampler call for the wrapped simulation: the parameter object as it is now, the Halton index carried on, the best
        path kept for iter_solution."""
        import torch
        _require_sampler_scope(self._parameter, self.obstacle_logic, self.dubins_paths and (rrt or self.dubins_leaf_scoring))
        e = self._ses.require_engine()
        self.set_parameter(self._parameter)
        sel = torch.zeros(1, dtype=torch.int32, device=e.device)
        start = torch.tensor([self.halton_next], dtype=torch.int32, device=e.device)
        o = run(e, sel, start)
        e.check_status()
        plan, n_act, result, nxt, nodes, n_nodes = e.fetch(o["plan"], o["n_actions"], o["result"], o["halton_next"], o["nodes"], o["n_nodes"])
        self.halton_next = int(nxt[0])
        last = None if rrt else best_leaf_node(e, self._parameter, o, nodes[0, :int(n_nodes[0])])
        self._solution = solution_edges(e, self._parameter, plan[0, :int(n_act[0])], nodes[0, :int(n_nodes[0])], last)
        return OptimizationResult(int(result[0]))

    def optimize2(self, slam, virtual_map):
        """EMPlanner2D::optimize2 (Planner2D.cpp:1043-1128) for the wrapped simulation: `drlgx_em_plan` under the two EM
        algorithms, `drlgx_og_plan` with the parameter's `alpha` under OG_SHANNON and SLAM_OG_SHANNON (non-Dubins control model
        only)."""
        return self._tree_call(lambda e, sel, start: plan_trees(e, self._parameter, sel, start, self.MAX_TREE_NODES, want_nodes=True))

    def rrt_planner(self, slam, virtual_map, n_key, fron_0, fron_1):
        """EMPlanner2D::rrt_planner (Planner2D.cpp:838-935): goal = node `n_key` of the pose graph if it is one, else the frontier
        point (fron_0, fron_1) (`drlgx_rrt_plan`)."""
        import torch

        def run(e, sel, start):
            key = torch.tensor([int(n_key)], dtype=torch.int32, device=e.device)
            xy = torch.tensor([[float(fron_0), float(fron_1)]], dtype=torch.float64, device=e.device)
            return e.rrt_plan(sel, key, xy, start, self.MAX_TREE_NODES, want_nodes=True)
        return self._tree_call(run, rrt=True)

    def iter_solution(self):
        """The edges of the best path from the best node back to the root (EMPlanner2D::BackwardIterator, Planner2D.h:200-257), each
        with `first` (the parent node), `second` (the node) and `get_odoms()`; callers insert at the front to get the plan."""
        return iter(self._solution)

    def _out_of_scope(self, *a, **k):
        raise NotImplementedError("optimize (RRT*), the Dubins library (without the opt-in dubins_paths) and iter_rrt are outside "
                                  "the accelerated path")

    optimize = iter_rrt = _out_of_scope

    def iter_dubins_library(self):
        """The Dubins library in library order (src/Planner2D.cpp:101-103), as the engine built it."""
        if not self.dubins_paths:
            self._out_of_scope()
        return iter(dubins_library(self._ses.require_engine()))

    def get_dubins_path(self, *index):
        """EMPlanner2D::getDubinsPath(i): entry `i` of the library."""
        if not self.dubins_paths:
            self._out_of_scope()
        return dubins_library(self._ses.require_engine())[int(index[0])]


def plan_trees(engine, parameter, env_sel, halton_start, max_tree_nodes, want_nodes=False):
    """optimize2's engine call for the parameter's algorithm: Engine.em_plan for EM_AOPT / EM_DOPT, Engine.og_plan with the
    parameter's alpha for OG_SHANNON / SLAM_OG_SHANNON (where the Dubins control model stays out of scope)."""
    alg = int(parameter.algorithm)
    if alg not in (int(OptimizationAlgorithm.OG_SHANNON), int(OptimizationAlgorithm.SLAM_OG_SHANNON)):
        return engine.em_plan(env_sel, halton_start, max_tree_nodes, alg, want_nodes=want_nodes)
    if parameter.dubins_control_model_enabled:
        raise NotImplementedError("optimize2 under OG_SHANNON / SLAM_OG_SHANNON runs the non-Dubins control model only")
    return engine.og_plan(env_sel, halton_start, max_tree_nodes, alg, float(parameter.alpha), want_nodes=want_nodes)


def load_dubins_library(engine, dubins_parameter):
    """Engine.set_dubins_library unless the engine already holds the library of these nine values."""
    if dubins_parameter is None:
        raise ValueError("dubins_control_model_enabled needs parameter.dubins_parameter (the [Dubins] section)")
    vals = tuple(float(getattr(dubins_parameter, f)) for f in engine.DUBINS_FIELDS)
    if engine.dubins_parameter != vals:
        engine.set_dubins_library(vals)


def dubins_library(engine):
    """The engine's library as a list of Dubins."""
    from . import ss2d
    lib = engine.dubins_library()
    return [Dubins(lib["v"][i], lib["w"][i], ss2d.Pose2(*lib["end"][i]), lib["num_steps"][i]) for i in range(len(lib["v"]))]


def _require_sampler_scope(parameter, obstacle_logic=False, dubins_rrt=False):
    """The sampler serves the non-Dubins control model at safe_distance = 0 (the engine refuses anything else with
    DRLGX_E_INVALID); the facades say so the way they say it for everything outside the accelerated path.  With `obstacle_logic`
    (the opt-in) any safe_distance >= 0 passes; the Dubins control model raises unless `dubins_rrt`: the caller is rrt_planner and
    has opted in to Dubins paths - or optimize2 and has opted in to the Dubins leaf scoring as well."""
    if parameter.dubins_control_model_enabled and not dubins_rrt:
        raise NotImplementedError("the tree sampler runs the Dubins control model for rrt_planner behind the opt-in "
                                  "dubins_paths=True, and for optimize2 behind dubins_paths=True with dubins_leaf_scoring=True")
    if obstacle_logic:
        if parameter.safe_distance < 0:
            raise ValueError("safe_distance must not be negative")
    elif parameter.safe_distance != 0:
        raise NotImplementedError("the tree sampler runs for the non-Dubins control model at safe_distance = 0 only "
                                  "(obstacle logic is an opt-in: obstacle_logic=True; Dubins paths are outside the accelerated path)")


class Node(object):
    """EMPlanner2D::Node as the binding shows it (src/Planner2D.cpp:51-60): key, state, poses, distance."""

    def __init__(self, key, pose, distance, poses=None):
        from . import ss2d
        self.key, self.distance = int(key), float(distance)
        self.state = ss2d.VehicleBeliefState(pose)
        self.poses = poses if poses is not None else ([pose] if key >= 0 else [])


class Edge(object):
    """EMPlanner2D::Edge (Planner2D.h:128-152): `get_odoms()` = the odometry from `first` to each pose of `second` - one pose, the
    edge's action, for the non-Dubins control model; one odometry per step, the origin moving along, for the Dubins model."""

    def __init__(self, first, second, odom):
        self.first, self.second, self._odoms = first, second, odom if isinstance(odom, list) else [odom]

    def get_odoms(self):
        return list(self._odoms)


def solution_edges(engine, parameter, plan, nodes, last=None):
    """The best path's edges, leaf first, for the control model of `parameter`; last: the path's last node under the Dubins model
    (None: the tree's last node, rrt_planner's goal)."""
    if parameter.dubins_control_model_enabled:
        return _dubins_solution_edges(engine, parameter, plan, nodes, last)
    return _solution_edges(engine, plan, nodes)


def best_leaf_node(engine, parameter, out, nodes):
    """optimize2 under the Dubins model, one tree: the node of the leaf em_plan picked - the leaves are the childless nodes in node
    order, and the picked one is the first whose per-step rows are the plan's, bit for bit.  None for the other control model (the
    plan's rows are the nodes' own columns there) and for an empty plan."""
    if not parameter.dubins_control_model_enabled or int(out["n_actions"][0]) == 0:
        return None
    lv = engine.em_plan_leaves()
    same = ((lv["actions"] == out["plan"][0]).flatten(1).all(dim=1) & (lv["n_actions"] == out["n_actions"][0])).nonzero().flatten()
    if same.numel() == 0:
        raise RuntimeError("the plan is not a leaf of the returned tree")
    parents = set(int(p) for p in nodes[1:, 3])
    return [j for j in range(len(nodes)) if j not in parents][int(same[0])]


def _dubins_solution_edges(engine, parameter, plan, nodes, last=None):
    """The Dubins model: the path ends at node `last` - rrt_planner's goal node is the last node of the tree when there is a plan;
    a node's columns 5-7 are (library index, num_steps, 0) and the plan holds one row per step, root -> `last`.  A node's poses
    are its steps from the parent's pose (connectNodeDubinsPath, Planner2D.cpp:157-176)."""
    from . import ss2d
    if len(plan) == 0:
        return []
    lib = engine.dubins_library()
    dt = float(parameter.dubins_parameter.dt)
    root_key = engine.counts(0)["poses"] - 1
    path = [len(nodes) - 1 if last is None else int(last)]
    while path[-1] > 0:
        path.append(int(nodes[path[-1], 3]))
    path.reverse()  # root .. goal
    if sum(int(nodes[j, 6]) for j in path[1:]) != len(plan):
        raise RuntimeError("the plan is not the path to the tree's last node")
    made = {0: Node(root_key, ss2d.Pose2(nodes[0, 0], nodes[0, 1], nodes[0, 2]), nodes[0, 4])}
    edges, row = [], 0
    for par, j in zip(path[:-1], path[1:]):
        m, ns = int(nodes[j, 5]), int(nodes[j, 6])
        v, w = float(lib["v"][m]), float(lib["w"][m])
        x, y, th = float(nodes[par, 0]), float(nodes[par, 1]), float(nodes[par, 2])
        poses = []
        for _ in range(ns):
            x, y, th = x + v * dt * math.cos(th), y + v * dt * math.sin(th), math.atan2(math.sin(th), math.cos(th)) + w * dt
            poses.append(ss2d.Pose2(x, y, math.atan2(math.sin(th), math.cos(th))))
        made[j] = Node(made[par].key + ns, ss2d.Pose2(nodes[j, 0], nodes[j, 1], nodes[j, 2]), nodes[j, 4], poses)
        edges.insert(0, Edge(made[par], made[j], [ss2d.Pose2(*plan[row + s]) for s in range(ns)]))
        row += ns
    return edges


def _solution_edges(engine, plan, nodes):
    """The best path's edges, leaf first: the path is found by walking the parents of the node whose edges are `plan`."""
    from . import ss2d
    if len(plan) == 0:
        return []
    root_key = engine.counts(0)["poses"] - 1
    # the best node: the one whose ancestors' edges are the plan (bit-equal columns 5..7), searched from the back
    depth = {0: 0}
    for j in range(1, len(nodes)):
        depth[j] = depth[int(nodes[j, 3])] + 1
    best = -1
    for j in range(len(nodes) - 1, 0, -1):
        if depth[j] != len(plan):
            continue
        k, q = j, len(plan) - 1
        while k > 0 and (nodes[k, 5:8] == plan[q]).all():
            k, q = int(nodes[k, 3]), q - 1
        if k == 0:
            best = j
            break
    if best < 0:
        raise RuntimeError("the plan is not a path of the returned tree")
    edges = []
    j = best
    while j > 0:
        par = int(nodes[j, 3])
        mk = lambda n: Node(root_key + depth[n] if n > 0 else root_key, ss2d.Pose2(nodes[n, 0], nodes[n, 1], nodes[n, 2]), nodes[n, 4])
        edges.append(Edge(mk(par), mk(j), ss2d.Pose2(nodes[j, 5], nodes[j, 6], nodes[j, 7])))
        j = par
    return edges
