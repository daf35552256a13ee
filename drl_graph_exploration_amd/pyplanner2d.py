"""Single-environment facades `SS2D` / `EMExplorer` with the reference's Python-wrapper surface
(scripts/envs/pyss2d.py:56-330, scripts/envs/pyplanner2d.py:57-84) over a one-env drlgx engine.

They exist so that code written against the reference wrappers (`ExplorationEnv`, notebooks, `test.py` reporting) can
run on the HIP path one environment at a time; throughput work should use `VecExplorationEnv`. The members the
reference's `ExplorationEnv` touches are provided:

    sim.simulate(odom)  sim.calculate_utility(d)  sim.line_plan(goal_key, fro)  sim.simulations_reward(actions)
    sim.plan()  sim.rrt_plan(goal_key, fro)  sim._planner.iter_solution()
    sim.step  sim.vehicle_position  sim.environment.get_landmark(key)
    sim._slam.key_size() / adjacency_degree_get() / adjacency_out() / features_out() / get_key_points(i)
    sim._slam.map.get_landmark_size() / iter_landmarks() / iter_trajectory() / get_current_vehicle()
    sim._virtual_map.to_array() / to_cov_trace() / explored() / get_parameter()
    sim._planner_params / _environment_params / _map_params / _virtual_map_params / _sensor_params / _control_params

`move / measure / optimize / update_virtual_map` are one fused device step and are not exposed separately.
"""
import math
from configparser import ConfigParser

import numpy as np
import torch

from . import planner2d, ss2d
from .config import DrlgxConfig, start_pose
from .engine import Engine


def load_config(path):
    cp = ConfigParser(inline_comment_prefixes=(";",))
    cp.read(path)
    return cp


def config_from_ini(cp, max_poses=256, max_actions=None, max_snapshots=1):
    """The ini sections of pyss2d.py:10-55 + pyplanner2d.py:24-54 -> struct drlgx_config (plus the parameter objects)."""
    sp = ss2d.BearingRangeSensorModelParameter()
    sp.bearing_noise = math.radians(cp.getfloat("Sensor Model", "bearing_noise"))
    sp.range_noise = cp.getfloat("Sensor Model", "range_noise")
    sp.min_bearing = math.radians(cp.getfloat("Sensor Model", "min_bearing"))
    sp.max_bearing = math.radians(cp.getfloat("Sensor Model", "max_bearing"))
    sp.min_range = cp.getfloat("Sensor Model", "min_range")
    sp.max_range = cp.getfloat("Sensor Model", "max_range")
    cm = ss2d.SimpleControlModelParameter()
    cm.rotation_noise = math.radians(cp.getfloat("Control Model", "rotation_noise"))
    cm.translation_noise = cp.getfloat("Control Model", "translation_noise")
    ep = ss2d.EnvironmentParameter()
    for k in ("min_x", "max_x", "min_y", "max_y", "max_steps", "safe_distance"):
        setattr(ep, k, cp.getfloat("Environment", k))
    mp = ss2d.EnvironmentParameter()
    ext = 20.0  # read_map_params(config, ext=20.0)
    mp.min_x, mp.max_x, mp.min_y, mp.max_y = ep.min_x - ext, ep.max_x + ext, ep.min_y - ext, ep.max_y + ext
    mp.safe_distance = ep.safe_distance
    vp = ss2d.VirtualMapParameter(mp)
    vp.resolution = cp.getfloat("Virtual Map", "resolution")
    vp.sigma0 = cp.getfloat("Virtual Map", "sigma0")
    vp.num_samples = cp.getint("Virtual Map", "num_samples")
    pp = planner2d.EMPlannerParameter()
    if cp.has_section("Planner"):
        for k in ("angle_weight", "distance_weight0", "distance_weight1", "d_weight", "max_edge_length", "occupancy_threshold",
                  "safe_distance", "max_nodes", "alpha"):
            if cp.has_option("Planner", k):
                setattr(pp, k, cp.getfloat("Planner", k))
        pp.seed = cp.getint("Planner", "seed")
        pp.reg_out = cp.getboolean("Planner", "reg_out")
        pp.algorithm = planner2d.OptimizationAlgorithm[cp.get("Planner", "algorithm")]
        if cp.has_option("Planner", "dubins_control_model_enabled"):
            pp.dubins_control_model_enabled = cp.getboolean("Planner", "dubins_control_model_enabled")
        if pp.dubins_control_model_enabled and cp.has_section("Dubins"):  # read_dubins_params (scripts/envs/pyplanner2d.py:9-20)
            pp.dubins_parameter = planner2d.DubinsParameter()
            for k in ("max_w", "dw", "min_v", "max_v", "dv", "dt", "min_duration", "max_duration", "tolerance_radius"):
                setattr(pp.dubins_parameter, k, cp.getfloat("Dubins", k))
    c = DrlgxConfig()
    c.bearing_noise, c.range_noise = sp.bearing_noise, sp.range_noise
    c.min_bearing, c.max_bearing, c.min_range, c.max_range = sp.min_bearing, sp.max_bearing, sp.min_range, sp.max_range
    c.translation_noise, c.rotation_noise = cm.translation_noise, cm.rotation_noise
    c.env_min_x, c.env_max_x, c.env_min_y, c.env_max_y, c.safe_distance = ep.min_x, ep.max_x, ep.min_y, ep.max_y, ep.safe_distance
    c.map_min_x, c.map_max_x, c.map_min_y, c.map_max_y = mp.min_x, mp.max_x, mp.min_y, mp.max_y
    c.resolution, c.sigma0, c.num_samples = vp.resolution, vp.sigma0, vp.num_samples
    c.sigma_x0 = cp.getfloat("Simulator", "sigma_x0")
    c.sigma_y0 = cp.getfloat("Simulator", "sigma_y0")
    c.sigma_theta0 = math.radians(cp.getfloat("Simulator", "sigma_theta0"))
    fixed = []
    if cp.has_section("Landmarks") and cp.has_option("Landmarks", "x") and cp.has_option("Landmarks", "y"):  # pyss2d.py:107-115
        import ast
        fixed = list(zip(ast.literal_eval(cp.get("Landmarks", "x")), ast.literal_eval(cp.get("Landmarks", "y"))))
    c.num_landmarks = cp.getint("Simulator", "num") + len(fixed)
    c.angle_weight, c.distance_weight0, c.distance_weight1 = pp.angle_weight, pp.distance_weight0, pp.distance_weight1
    c.occupancy_threshold, c.max_edge_length, c.algorithm = pp.occupancy_threshold, pp.max_edge_length, int(pp.algorithm)
    c.max_poses = max_poses
    c.max_landmarks = max(1, min(c.num_landmarks, 127))
    c.max_factors = max(64, 12 * max_poses)
    if max_actions is None:  # the longest line plan the boxes allow (config.default_config)
        span = max(ep.max_x - ep.min_x, ep.max_y - ep.min_y, (mp.max_x - mp.min_x) / 2, (mp.max_y - mp.min_y) / 2)
        max_actions = int(math.ceil(math.hypot(span, span) / c.max_edge_length)) + 3
    c.max_actions, c.max_snapshots = max_actions, max_snapshots
    return c, dict(sensor=sp, control=cm, environment=ep, map=mp, virtual_map=vp, planner=pp, fixed_landmarks=fixed)


class _Map(object):
    """SLAM2D.map / Simulator2D.environment: an `Environment` view (src/SS2D.cpp:141-171)."""

    def __init__(self, owner, truth):
        self._o, self._truth = owner, truth

    def get_landmark_size(self):
        return self._o.engine.cfg.num_landmarks if self._truth else self._o.engine.counts(0)["landmarks"]

    def get_trajectory_size(self):
        return self._o.engine.counts(0)["poses"]

    @property
    def distance(self):
        """Environment::getDistance (Simulator2D.cpp:244-250)."""
        return ss2d.trajectory_distance([v.pose for v in self.iter_trajectory()])

    def iter_landmarks(self):
        if self._truth:
            _, lms = self._o.engine.ground_truth(0)
            for k, p in enumerate(lms):
                yield k, ss2d.LandmarkBeliefState(ss2d.Point2(*p))
        else:
            keys, xy, info = self._o.engine.landmarks(0)
            for k, p, i in zip(keys, xy, info):
                yield int(k), ss2d.LandmarkBeliefState(ss2d.Point2(*p), i)

    def get_landmark(self, key):
        for k, l in self.iter_landmarks():
            if k == key:
                return l
        raise KeyError(key)

    def iter_trajectory(self):
        if self._truth:
            veh, _ = self._o.engine.ground_truth(0)
            yield ss2d.VehicleBeliefState(ss2d.Pose2(*veh))
            return
        xyt, info = self._o.engine.poses(0)
        for p, i in zip(xyt, info):
            yield ss2d.VehicleBeliefState(ss2d.Pose2(*p), i)

    def get_current_vehicle(self):
        if self._truth:
            return next(self.iter_trajectory())
        xyt, info = self._o.engine.poses(0)
        return ss2d.VehicleBeliefState(ss2d.Pose2(*xyt[-1]), info[-1])


class _Slam(object):
    """SLAM2D getters used by graph_matrix (src/SLAM2D.cpp:141-273)."""

    def __init__(self, owner):
        self._o = owner
        self.map = _Map(owner, False)

    def key_size(self):
        c = self._o.engine.counts(0)
        return c["poses"] + c["landmarks"]

    def adjacency_degree_get(self):
        self._A, self._X = self._o.engine.adjacency(0)

    def adjacency_out(self):
        return self._A

    def features_out(self):
        return self._X.reshape(-1, 1)

    def get_key_points(self, i):
        keys, lxy, _ = self._o.engine.landmarks(0)
        if i < len(keys):
            return [lxy[i][0], lxy[i][1]]
        xyt, _ = self._o.engine.poses(0)
        return [xyt[i - len(keys)][0], xyt[i - len(keys)][1]]


class _VirtualMap(object):
    def __init__(self, owner):
        self._o = owner

    def to_array(self):
        return self._o.engine.virtual_map(0)[0]

    def to_cov_trace(self):
        return self._o.engine.virtual_map(0)[2]

    def to_cov_array(self):
        ln, an = self._o.engine.cov_array()
        return ln[0].cpu().numpy(), an[0].cpu().numpy()

    def explored(self):
        return float(self._o.engine.explored()[0])

    def get_parameter(self):
        return self._o._virtual_map_params


class _Sim(object):
    def __init__(self, owner):
        self._o = owner
        self.environment = _Map(owner, True)

    @property
    def vehicle(self):
        return ss2d.Pose2(*self._o.engine.ground_truth(0)[0])


class SS2D(object):
    """scripts/envs/pyss2d.py:56-330 (construction + simulate + getters).

    One fused device step per `simulate` (`drlgx_step`).  (The same simulation driven call by call through the `ss2d`
    module's own classes, in the reference's order, lives in tests/staged_facade.py - the module classes are the API, that
    driver is test code.)"""

    def __init__(self, config, verbose=False, device=0, max_poses=256, start=None):
        self._config = load_config(config) if isinstance(config, str) else config
        cfg, prm = config_from_ini(self._config, max_poses=max_poses)
        self._sensor_params, self._control_params = prm["sensor"], prm["control"]
        self._environment_params, self._map_params = prm["environment"], prm["map"]
        self._virtual_map_params, self._planner_params = prm["virtual_map"], prm["planner"]
        lo = int(self._config.getfloat("Simulator", "lo"))
        seed = self._config.getint("Simulator", "seed")
        # `start` (x, y, theta) overrides the reference's integer start pose (extension used by tests)
        x0, y0, theta0 = start_pose(lo, cfg.map_max_x) if start is None else start
        self.verbose = verbose
        self.engine = Engine(cfg, 1, max(cfg.max_landmarks, 1), device)
        if prm["fixed_landmarks"]:
            self.engine.set_fixed_landmarks(prm["fixed_landmarks"])
        self.engine.reset([0], [seed], starts=np.array([[x0, y0, theta0]]))
        self.engine.check_status()
        self._slam, self._virtual_map, self._sim = _Slam(self), _VirtualMap(self), _Sim(self)

    @property
    def step(self):
        return self.engine.counts(0)["step"]

    def simulate(self, odom, core=True):
        """pyss2d.py:171-206; returns True when the odometry is rejected (outside the map box)."""
        if not core:
            raise NotImplementedError("non-core (Dubins intermediate) steps are outside the accelerated path")
        mp = self._map_params
        if not mp.min_x < odom[0] < mp.max_x or not mp.min_y < odom[1] < mp.max_y:
            return True
        self.engine.step(torch.tensor([[odom[0], odom[1], odom[2]]], dtype=torch.float64, device=self.engine.device))
        self.engine.check_status()
        return False

    @property
    def vehicle_position(self):
        return self._slam.map.get_current_vehicle().pose

    @property
    def environment(self):
        return self._sim.environment

    @property
    def map(self):
        return self._slam.map

    @property
    def distance(self):
        """pyss2d.py:216-218: the travelled distance of the estimated trajectory."""
        return self._slam.map.distance


class _Planner(object):
    """`EMExplorer._planner`: what ExplorationEnv.plan / rrt_plan read after a successful call - `iter_solution()` - and the Halton
    index that carries on from call to call (started as the reference's constructor starts it)."""

    def __init__(self, owner):
        self._o = owner
        self.halton_next = planner2d.halton_start_index(owner._planner_params.seed)
        self._solution = []

    def _call(self, run, rrt=False):
        o, pp = self._o, self._o._planner_params
        planner2d._require_sampler_scope(pp, o.obstacle_logic, o.dubins_paths and (rrt or o.dubins_leaf_scoring))
        e = o.engine
        e.set_sampler_parameter(pp.max_nodes, pp.safe_distance, pp.dubins_control_model_enabled)
        e.set_sampler_obstacles(o.obstacle_logic)
        e.set_dubins_leaf_scoring(o.dubins_paths and o.dubins_leaf_scoring)
        if o.dubins_paths and pp.dubins_control_model_enabled:
            planner2d.load_dubins_library(e, pp.dubins_parameter)
        sel = torch.zeros(1, dtype=torch.int32, device=e.device)
        start = torch.tensor([self.halton_next], dtype=torch.int32, device=e.device)
        out = run(e, sel, start)
        plan, n_act, result, nxt, nodes, n_nodes = e.fetch(out["plan"], out["n_actions"], out["result"], out["halton_next"], out["nodes"],
                                                           out["n_nodes"])
        self.halton_next = int(nxt[0])
        last = None if rrt else planner2d.best_leaf_node(e, pp, out, nodes[0, :int(n_nodes[0])])
        self._solution = planner2d.solution_edges(e, pp, plan[0, :int(n_act[0])], nodes[0, :int(n_nodes[0])], last)
        self.last = out
        return planner2d.OptimizationResult(int(result[0]))

    def optimize2(self):
        cap = planner2d.EMPlanner2D.MAX_TREE_NODES
        return self._call(lambda e, sel, start: planner2d.plan_trees(e, self._o._planner_params, sel, start, cap, want_nodes=True))

    def rrt_planner(self, n_key, fron_0, fron_1):
        cap = planner2d.EMPlanner2D.MAX_TREE_NODES

        def run(e, sel, start):
            key = torch.tensor([int(n_key)], dtype=torch.int32, device=e.device)
            xy = torch.tensor([[float(fron_0), float(fron_1)]], dtype=torch.float64, device=e.device)
            return e.rrt_plan(sel, key, xy, start, cap, want_nodes=True)
        return self._call(run, rrt=True)

    def iter_solution(self):
        return iter(self._solution)

    def iter_dubins_library(self):
        if not self._o.dubins_paths:
            raise NotImplementedError("the Dubins library is an opt-in: dubins_paths=True")
        planner2d.load_dubins_library(self._o.engine, self._o._planner_params.dubins_parameter)
        return iter(planner2d.dubins_library(self._o.engine))

    def get_dubins_path(self, index):
        return list(self.iter_dubins_library())[int(index)]


class EMExplorer(SS2D):
    """scripts/envs/pyplanner2d.py:57-84.  `obstacle_logic` (an opt-in, off by default): plan() / rrt_plan() run the planner's
    safe_distance as the ini file gives it, with the sampler's obstacle logic (Engine.set_sampler_obstacles); off, a non-zero
    planner safe_distance raises NotImplementedError as before.  `dubins_paths` (an opt-in too): with `[Planner]
    dubins_control_model_enabled = true` rrt_plan() runs the Dubins control model with the ini file's [Dubins] library
    (Engine.set_dubins_library), an edge's get_odoms() then holds one odometry per step; plan() raises unless
    `dubins_leaf_scoring` (one more opt-in, Engine.set_dubins_leaf_scoring) is set as well: plan() then runs optimize2 with the
    Dubins tree and the leaf evaluation that knows non-core steps, and iter_solution() yields the best leaf's edges, one odometry
    per step; off, the flag raises NotImplementedError as before.  Executing the intermediate steps (simulate(core=False)) stays outside the accelerated path."""

    def __init__(self, *args, **kwargs):
        self.obstacle_logic = bool(kwargs.pop("obstacle_logic", False))
        self.dubins_paths = bool(kwargs.pop("dubins_paths", False))
        self.dubins_leaf_scoring = bool(kwargs.pop("dubins_leaf_scoring", False))
        self.env_obstacles = bool(kwargs.pop("env_obstacles", False))
        super(EMExplorer, self).__init__(*args, **kwargs)
        self._planner = _Planner(self)
        if self.env_obstacles:  # (after the reset: the latch starts up either way, pyss2d.py:132)
            self.engine.set_env_obstacles(True)

    def simulate(self, odom, core=True):
        """pyss2d.py:171-206.  `env_obstacles` (an opt-in, off by default: Engine.set_env_obstacles): True also when the step raised
        the obstacle flag of the ini file's [Environment] safe_distance; without it True for a rejected odometry only, as before."""
        if super(EMExplorer, self).simulate(odom, core):
            return True
        if not self.env_obstacles:
            return False
        (flag,) = self.engine.fetch(self.engine.obstacle_flags()[0])
        return bool(flag[0])

    def follow_path(self, steps=3):
        """pyplanner2d.py:100-109: the first `steps` edges of the last plan, root first; True when a step was rejected or - under
        `env_obstacles` - met an obstacle (the path is left there), None otherwise, as the reference."""
        if self._planner_params.dubins_control_model_enabled:
            raise NotImplementedError("follow_dubins_path executes intermediate poses with simulate(core=False), which is outside the "
                                      "accelerated path")
        path = []
        for edge in self._planner.iter_solution():
            path.insert(0, edge.get_odoms()[0])
        for odom in path[:steps]:
            if self.simulate((odom.x, odom.y, odom.theta), core=True):
                return True

    def plan(self):
        """pyplanner2d.py:70-71: EMPlanner2D::optimize2 on the device; the path is then `self._planner.iter_solution()`."""
        return self._planner.optimize2() == planner2d.OptimizationResult.SUCCESS

    def rrt_plan(self, goal_key, fron):
        """pyplanner2d.py:73-74: EMPlanner2D::rrt_planner to graph node `goal_key` if it is one, else to the point `fron`."""
        return self._planner.rrt_planner(goal_key, fron[0], fron[1]) == planner2d.OptimizationResult.SUCCESS

    def calculate_utility(self, distance):
        d = torch.tensor([float(distance)], dtype=torch.float64, device=self.engine.device)
        return float(self.engine.utility(d)[0])

    def line_plan(self, goal_key, fron):
        ce = torch.zeros(1, dtype=torch.int32, device=self.engine.device)
        goal = torch.tensor([[fron[0], fron[1]]], dtype=torch.float64, device=self.engine.device)
        acts, n = self.engine.line_plan(ce, goal)
        self._last_plan = (acts, n)
        return [ss2d.Pose2(*a) for a in acts[0, :int(n[0])].cpu().numpy()]

    def simulations_reward(self, actions):
        A = self.engine.cfg.max_actions
        acts = torch.zeros(1, A, 3, dtype=torch.float64, device=self.engine.device)
        for k, a in enumerate(actions):
            acts[0, k] = torch.tensor([a.x, a.y, a.theta] if hasattr(a, "x") else list(a), dtype=torch.float64)
        n = torch.tensor([len(actions)], dtype=torch.int32, device=self.engine.device)
        ce = torch.zeros(1, dtype=torch.int32, device=self.engine.device)
        return float(self.engine.lookahead(ce, acts, n)[0])


def explore(config_file, max_distance=450, verbose=False, save_history=False, save_fig=False):
    """scripts/envs/pyplanner2d.py:155-195: four scanning turns, then plan / follow_path(5) until the planner reports NO_SOLUTION or
    TERMINATION, 200 steps have passed or the travelled distance exceeds `max_distance`; returns (status, mean planning time).
    The planner's obstacle logic and SS2D.simulate's obstacle flag are switched on from the ini file's [Planner] and [Environment]
    safe_distance.  The switch reads the planner's result itself (the reference compares plan()'s bool with the enum, so its first
    three branches never run).  Plots and history dumps are out of scope: save_fig / save_history raise."""
    from time import time
    if save_fig or save_history:
        raise NotImplementedError("explore(): plots (save_fig) and .npz history dumps (save_history) are out of scope")
    cp = load_config(config_file) if isinstance(config_file, str) else config_file
    _, prm = config_from_ini(cp)
    explorer = EMExplorer(cp, verbose, obstacle_logic=prm["planner"].safe_distance != 0.0,
                          env_obstacles=prm["environment"].safe_distance > 0.0)
    status = 'MAX_DISTANCE'
    planning_count = 0
    planning_time = 0.0
    try:
        for step in range(200):
            if step < 4:
                explorer.simulate((0, 0, math.pi / 2.0), core=True)
            else:
                start = time()
                result = explorer._planner.optimize2()
                planning_time += time() - start
                planning_count += 1
                if result == planner2d.OptimizationResult.SAMPLING_FAILURE:
                    explorer.simulate((0, 0, math.pi / 4), True)
                elif result == planner2d.OptimizationResult.NO_SOLUTION:
                    status = 'NO SOLUTION'
                    break
                elif result == planner2d.OptimizationResult.TERMINATION:
                    status = 'TERMINATION'
                    break
                else:
                    explorer.follow_path(5)
                if explorer.distance > max_distance:
                    break
    finally:
        explorer.engine.close()
    return status, planning_time / max(planning_count, 1)
