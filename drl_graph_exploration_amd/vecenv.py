"""`VecExplorationEnv` — the batched counterpart of the reference's `ExplorationEnv`
(scripts/envs/exploration_env.py:20-422): `n_envs` independent exploration environments stepped in lock-step on one
GPU through the drlgx engine (one workgroup per environment per kernel).

Method names and meaning follow the reference class; everything that was a scalar / list per environment becomes a
device tensor over environments (or over (environment, frontier) candidates):

    reset()              ExplorationEnv.reset      (:389-422)  SS2D.__init__, 4 x (1, 1, pi/2), regenerate (+50) if no landmark
    graph_matrix()       frontier + graph_matrix + DeepQ.data_process (:196-348, policy.py:211-232) -> one PyG-style batch
    actions_all_goals()  (:134-143)  line plan to every frontier of every env
    rewards_all_goals()  (:145-162)  look-ahead reward of every plan + the per-decision np.interp normalisation / loop_clo
    step(...)            (:98-105)   executes one chosen plan per env (ragged lengths -> active masks)
    step_traced(...)     the same plans as scripts/test.py:128-152 executes them: a metric row per action, stop at done
    status() / done()    (:164-168, :107-110)

There is no CPU path here: the engine raises if no HIP device is visible.
"""
import math

import numpy as np
import torch

from .config import default_config, start_pose
from .engine import Engine


def normalise_rewards(raw, cand_env, cand_first, n_envs, n_frontier=None):
    """exploration_env.py:151-161 for every env at once. raw [C] f64 look-ahead rewards of the (env, frontier)
    candidates in env-major order, cand_env [C] i64, cand_first [n_envs] i64 (index of each env's frontier 0 = the
    vehicle's nearest frontier). Returns (normalised [C], loop_clo [n_envs] bool): the nearest frontier is the
    (first) arg-max -> np.interp to [-1, 0], loop_clo False; otherwise [-1, 1], loop_clo True.
    Device tensors go through drlgx_normalise_rewards (one wave per env); the tensor-op form below is the host mirror the
    CPU tests check against np.interp."""
    if raw.is_cuda:
        import ctypes as C
        from . import _lib
        if n_frontier is None:
            n_frontier = torch.diff(torch.cat([cand_first, torch.tensor([raw.numel()], device=raw.device)])).to(torch.int32)
        raw = raw.contiguous()
        out = torch.empty_like(raw)
        loop = torch.empty(n_envs, dtype=torch.uint8, device=raw.device)
        vp = C.c_void_p
        _lib.check(_lib.lib().drlgx_normalise_rewards(vp(_lib.stream_ptr(raw.device)), n_envs, vp(raw.data_ptr()),
                                                      vp(cand_first.contiguous().data_ptr()), vp(n_frontier.contiguous().data_ptr()),
                                                      vp(out.data_ptr()), vp(loop.data_ptr())))
        return out, loop.bool()
    e = cand_env
    lo = torch.full((n_envs,), float("inf"), dtype=raw.dtype, device=raw.device).scatter_reduce(0, e, raw, reduce="amin")
    hi = torch.full((n_envs,), -float("inf"), dtype=raw.dtype, device=raw.device).scatter_reduce(0, e, raw, reduce="amax")
    nearest = raw[cand_first.clamp(max=max(raw.numel() - 1, 0))]
    loop_clo = nearest < hi  # np.nanargmax returns the first maximum
    top = torch.where(loop_clo, 1.0, 0.0).to(raw.dtype)
    span = hi - lo
    slope = (top + 1.0) / torch.where(span > 0, span, torch.ones_like(span))
    r = slope[e] * (raw - lo[e]) - 1.0  # np.interp: slope * (x - xp[0]) + fp[0]
    r = torch.where(raw >= hi[e], top[e], r)  # x >= xp[-1] -> fp[-1] (also the degenerate lo == hi case)
    return r, loop_clo


class VecExplorationEnv(object):
    def __init__(self, map_size, n_envs, env_index=0, test=True, num_landmarks=None, algorithm=0, device=0,
                 n_rollouts=None, max_poses=None, starts=None, seed=None, alpha=None):
        self.map_size = map_size
        # the planner parameter alpha (SLAM_OG_SHANNON's weight of the landmark term; None: EMPlannerParameter's default)
        from .planner2d import EMPlannerParameter
        self.alpha = EMPlannerParameter().alpha if alpha is None else float(alpha)
        self.n_envs = n_envs
        self.test = test
        if max_poses is None:
            # the reference's own 40 m evaluation episodes take 96-197 primitive steps (data/test_result/40_DQN_GCN.csv)
            # on top of the 5 poses of reset().  The capacity costs memory only: the engine picks the SLAM kernel per
            # launch from the trajectories' current length (fused LDS-resident step up to 42 poses, the pose-chain
            # ordered solve of csrc/k_slam_arrow.hip beyond), refreshed at every status check
            max_poses = 256
        self.cfg = default_config(map_size, num_landmarks=num_landmarks, algorithm=algorithm, max_poses=max_poses)
        if n_rollouts is None:
            # one rollout instance per (env, frontier) candidate up to 4096; more candidates run in waves
            n_rollouts = min(n_envs * (self.cfg.max_landmarks + 1), 4096)
        self.engine = Engine(self.cfg, n_envs, n_rollouts, device)
        self.device = self.engine.device
        self.np_random = np.random.RandomState(seed)
        if np.ndim(env_index) == 0:
            self.env_index = np.arange(n_envs, dtype=np.int64) + int(env_index)  # one TEST seed per env
        else:  # (the seeds listed one by one)
            self.env_index = np.array(env_index, dtype=np.int64).reshape(n_envs)
        self._starts = None if starts is None else np.asarray(starts, dtype=np.float64).reshape(n_envs, 3)
        self._max_steps = 5000
        self.dist = torch.zeros(n_envs, dtype=torch.float64, device=self.device)
        self.loop_clo = torch.zeros(n_envs, dtype=torch.bool, device=self.device)
        self._graph = None
        self._cand_env = None
        self._scan = torch.tensor([(1.0, 1.0, math.pi / 2.0)] * n_envs, dtype=torch.float64, device=self.device)
        self.reset()

    def close(self):
        self.engine.close()

    # ------------------------------------------------------------------ reset (exploration_env.py:389-422)
    def reset(self, ids=None):
        """Re-create the listed environments (all by default)."""
        n = self.n_envs
        todo = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
        self.dist[torch.as_tensor(todo, device=self.device)] = 0.0
        if getattr(self, "_halton_next", None) is not None:  # (a re-created env gets a new planner: its Halton index starts over)
            self._halton_next = self._halton_next.clone()
            self._halton_next[torch.as_tensor(todo, device=self.device)] = self._halton_start
        while len(todo):
            if self.test:
                seeds = self.env_index[todo].astype(np.uint32)
                los = self.env_index[todo]
            else:
                hi = np.iinfo(np.int32).max
                seeds = np.array([self.np_random.randint(0, hi) for _ in todo], dtype=np.uint32)
                los = np.array([self.np_random.randint(0, hi) for _ in todo], dtype=np.int64)
            if self._starts is not None:
                starts = self._starts[todo]
            else:
                starts = np.array([start_pose(int(lo), self.cfg.map_max_x) for lo in los], dtype=np.float64)
            self.engine.reset(todo.astype(np.int32), seeds, starts=starts)
            active = torch.zeros(n, dtype=torch.uint8, device=self.device)
            active[torch.as_tensor(todo, device=self.device)] = 1
            for _ in range(4):
                self.engine.step(self._scan, active)
            (n_lm,) = self.engine.fetch(self.engine.counts_dev()[:, 1])  # (with the status check, one synchronisation)
            empty = np.array([i for i in todo if n_lm[i] < 1], dtype=np.int64)
            self.env_index[empty] += 50  # "regenerate a environment"
            todo = empty
        self._graph = None
        return self._get_obs()

    def _get_obs(self):
        return None  # the occupancy grids stay on the device; use obs(i) for one env's VirtualMap.to_array()

    def obs(self, i):
        return self.engine.virtual_map(int(i))[0]

    # ------------------------------------------------------------------ graph export
    def graph_matrix(self, plan=False):
        """All envs' graphs as one batch (see Engine.graph); node order per env = [landmarks (hash order), poses,
        frontiers], edge order = DeepQ.data_process's. Candidate c = (env, frontier) in env-major order.
        plan=True (the trainers): the line plans to all frontiers come out of the same call and the same synchronisation
        (Engine.graph(plan=True)); actions_all_goals() then has nothing left to do."""
        g = self.engine.graph(plan=plan)  # (one synchronisation: the status word, the batch's boundaries and the frontier counts)
        nfr_h = g["n_frontier_h"].astype(np.int64)
        n_cand = int(nfr_h.sum())
        self._graph = g
        # the candidate arrays are host arithmetic on the frontier counts: one upload instead of a dozen small launches
        first_h = np.cumsum(nfr_h) - nfr_h
        env_h = np.repeat(np.arange(self.n_envs, dtype=np.int64), nfr_h)
        fidx_h = np.arange(n_cand, dtype=np.int64) - first_h[env_h]
        node_h = g["node_off_h"][1:].astype(np.int64)[env_h] - nfr_h[env_h] + fidx_h  # node_off[e+1] - n_frontier[e] + f
        mf = g["frontier_xy"].shape[1]
        up = torch.as_tensor(np.concatenate([env_h, fidx_h, node_h, env_h * mf + fidx_h, first_h]), device=self.device)
        env_t, fidx, node_t, slot_t, first = (up[:n_cand], up[n_cand:2 * n_cand], up[2 * n_cand:3 * n_cand], up[3 * n_cand:4 * n_cand],
                                              up[4 * n_cand:])
        self._cand_env = env_t.to(torch.int32)
        self._cand_first, self._cand_first_h = first, first_h
        self._cand_fidx = fidx
        self._cand_node = node_t
        self._goals = g["frontier_xy"].view(-1, 2)[slot_t].contiguous()
        self._n_act_h = None
        self._actions = self._n_act = None
        if plan:
            self._actions = g["actions_pad"].view(self.n_envs * mf, -1, 3)[slot_t].contiguous()
            self._n_act = g["n_act_pad"].view(-1)[slot_t].contiguous()
            self._n_act_h = g["n_act_pad_h"].reshape(-1)[env_h * mf + fidx_h]
        return g

    @property
    def candidates(self):
        """(cand_env [C] i32, cand_node [C] i64 global node ids, first candidate of each env [n_envs] i64)."""
        return self._cand_env, self._cand_node, self._cand_first

    def actions_all_goals(self):
        """Line plan to every frontier: (actions [C, max_actions, 3] f64, n_actions [C] i32)."""
        if self._graph is None:
            self.graph_matrix()
        if self._actions is not None:  # (graph_matrix(plan=True) planned already)
            return self._actions, self._n_act
        self._actions, self._n_act = self.engine.line_plan(self._cand_env, self._goals)
        # the plans' lengths on the host: the look-ahead and the step launch the action indices some plan reaches
        (self._n_act_h,) = self.engine.fetch(self._n_act)
        return self._actions, self._n_act

    # ------------------------------------------------------------------ the EM-exploration baseline (exploration_env.py:107-128)
    def _halton(self, seed):
        from .planner2d import halton_start_index
        if getattr(self, "_halton_next", None) is None:  # every env's planner starts where the reference's constructor starts it
            self._halton_start = halton_start_index(seed)
            self._halton_next = torch.full((self.n_envs,), self._halton_start, dtype=torch.int32, device=self.device)
        return self._halton_next

    def _with_safe_distance(self, max_nodes, safe_distance, run):
        """One sampler call under `safe_distance` (None: the engine's settings as they are, only max_nodes replaced if given): a
        value opts in to the sampler's obstacle logic for this call, and the engine's previous sampler settings come back after it."""
        e = self.engine
        old_par, old_obs = e.sampler_parameter, e.sampler_obstacles
        if safe_distance is None:
            if max_nodes is not None:
                e.set_sampler_parameter(max_nodes)
            return run()
        e.set_sampler_parameter(old_par[0] if max_nodes is None else max_nodes, safe_distance)
        e.set_sampler_obstacles(True)
        try:
            return run()
        finally:
            e.set_sampler_parameter(*old_par)
            e.set_sampler_obstacles(old_obs)

    def _with_dubins(self, dubins, leaf_scoring, run):
        """`run` under the Dubins control model with the library of `dubins` (Engine.set_dubins_library, kept loaded for the next
        such call) and - leaf_scoring - the opt-in of em_plan; the engine's Dubins flag and that opt-in come back after it."""
        from .planner2d import load_dubins_library

        def wrapped():
            e = self.engine
            load_dubins_library(e, dubins)
            now, old_ls = e.sampler_parameter, e.dubins_leaf_scoring
            e.set_sampler_parameter(now[0], now[1], True)
            if leaf_scoring:
                e.set_dubins_leaf_scoring(True)
            try:
                return run()
            finally:
                e.set_sampler_parameter(*now)
                if leaf_scoring:
                    e.set_dubins_leaf_scoring(old_ls)
        return wrapped

    def em_plan(self, max_nodes=0.5, max_tree_nodes=2048, planner_seed=0, safe_distance=None, dubins=None):
        """ExplorationEnv.plan for all envs in one call (EMPlanner2D::optimize2; Engine.em_plan under the EM algorithms, Engine.og_plan
        with the planner parameter `alpha` (self.alpha) under OG_SHANNON / SLAM_OG_SHANNON): per env the tree, the leaves' expected
        costs with the configured algorithm, the best leaf's action list.  Returns (actions [n_envs, max_actions, 3] f64 edge
        odometry, n_actions [n_envs] i32, result [n_envs] i32) on the device; every env's Halton index carries on from call to
        call.  `safe_distance` (None: 0, as before): a value runs this call with the sampler's obstacle logic at that planner
        safe_distance (an env can then have result SAMPLING_FAILURE and no actions) and restores the engine's sampler settings.
        `dubins` (a planner2d.DubinsParameter; None: the non-Dubins control model as before): this call runs optimize2 under the
        Dubins control model with that library - it sets the library, the Dubins flag and the opt-in of the Dubins leaf scoring
        (Engine.set_dubins_leaf_scoring), the actions are then one odometry per step, an env can have result SAMPLING_FAILURE -
        and the engine's Dubins flag and opt-in come back after it (EM algorithms only: the OG algorithms refuse `dubins`)."""
        sel = torch.arange(self.n_envs, dtype=torch.int32, device=self.device)
        start = self._halton(planner_seed)
        alg = int(self.cfg.algorithm)
        if alg in (2, 3):  # OG_SHANNON, SLAM_OG_SHANNON
            if dubins is not None:
                raise NotImplementedError("optimize2 under OG_SHANNON / SLAM_OG_SHANNON runs the non-Dubins control model only")
            run = lambda: self.engine.og_plan(sel, start, max_tree_nodes, alg, self.alpha)
        else:
            run = lambda: self.engine.em_plan(sel, start, max_tree_nodes, alg)
        if dubins is not None:
            run = self._with_dubins(dubins, True, run)
        o = self._with_safe_distance(max_nodes, safe_distance, run)
        self._halton_next = o["halton_next"]
        return o["plan"], o["n_actions"], o["result"]

    def rrt_plan(self, goal_key, frontier, max_tree_nodes=2048, planner_seed=0, safe_distance=None, dubins=None):
        """ExplorationEnv.rrt_plan for all envs in one call (EMPlanner2D::rrt_planner, Engine.rrt_plan): goal_key [n_envs] i32 (a graph
        node if it is one), frontier [n_envs, 2] f64 (the goal otherwise), on the device.  Returns like em_plan; an env whose tree
        fills max_tree_nodes before it reaches the goal has result SAMPLING_FAILURE and no actions.  `safe_distance`: as em_plan's
        (a goal whose edge is unsafe gives SUCCESS with no actions, as the reference's empty solution).  `dubins` (a
        planner2d.DubinsParameter; None: the non-Dubins control model as before): this call runs the Dubins control model with that
        library (Engine.set_dubins_library, kept loaded for the next such call) - the actions are then one odometry per step - and
        the engine's Dubins flag comes back after it."""
        sel = torch.arange(self.n_envs, dtype=torch.int32, device=self.device)
        start = self._halton(planner_seed)
        run = lambda: self.engine.rrt_plan(sel, goal_key.to(torch.int32).contiguous(), frontier.to(torch.float64).contiguous(), start,
                                           max_tree_nodes)
        if dubins is not None:
            run = self._with_dubins(dubins, False, run)
        o = self._with_safe_distance(None, safe_distance, run)
        self._halton_next = o["halton_next"]
        return o["plan"], o["n_actions"], o["result"]

    def rewards_all_goals(self, all_actions=None, return_raw=False, lookahead="sim"):
        """Look-ahead reward per candidate, normalised per env like exploration_env.py:151-161:
        nearest frontier is the arg-max -> interp to [-1, 0], loop_clo False; else [-1, 1], loop_clo True.
        lookahead="sim": the stochastic look-ahead (EMPlanner2D::simulations_reward, drlgx_lookahead).  "em": the deterministic
        expected cost instead - raw = the root's uncertainty (Engine.uncertainty_em) minus the leaf's cost (Engine.em_cost, the
        leaf evaluation of optimize2) with the planner parameter's algorithm: the sign convention of U_before - U_after.  "og":
        the expected map entropy (Engine.og_cost, calculateUncertainty_OG_SHANNON) in the same convention - raw = the entropy of
        the candidate's environment with no action (one extra candidate per env in the same call) minus the candidate's cost.
        "slam_og": the SLAM-OG-Shannon cost (Engine.slam_og_cost, calculateUncertainty_SLAM_OG_SHANNON) exactly as "og" - raw = the
        uncertainty of the environment with no action minus the candidate's cost - with the planner parameter `alpha` (self.alpha)."""
        if lookahead not in ("sim", "em", "og", "slam_og"):
            raise ValueError("lookahead must be 'sim', 'em', 'og' or 'slam_og', not %r" % (lookahead,))
        actions, n_act = all_actions if all_actions is not None else (self._actions, self._n_act)
        if lookahead in ("og", "slam_og"):
            nc = self._cand_env.numel()
            roots = torch.arange(self.n_envs, dtype=torch.int32, device=self.device)
            cands = (torch.cat([self._cand_env, roots]), torch.cat([actions, actions.new_zeros((self.n_envs,) + tuple(actions.shape[1:]))]),
                     torch.cat([n_act, torch.zeros_like(roots)]))
            ent, cost = self.engine.og_cost(*cands) if lookahead == "og" else self.engine.slam_og_cost(*cands, self.alpha)
            raw = ent[nc:][self._cand_env.long()] - cost[:nc]
            r, self.loop_clo = normalise_rewards(raw, self._cand_env.long(), self._cand_first, self.n_envs, self._graph["n_frontier"])
            return (r, raw) if return_raw else r
        if lookahead == "em":
            alg = int(self.cfg.algorithm)
            _, cost = self.engine.em_cost(self._cand_env, actions, n_act, alg)
            raw = self.engine.uncertainty_em(alg)[self._cand_env.long()] - cost
            r, self.loop_clo = normalise_rewards(raw, self._cand_env.long(), self._cand_first, self.n_envs, self._graph["n_frontier"])
            return (r, raw) if return_raw else r
        n_act_h = self._n_act_h if all_actions is None else None
        if n_act_h is not None:
            kmax = max(int(n_act_h.max()), 1) if n_act_h.size else 1
        else:
            kmax = max(int(n_act.max().item()), 1) if n_act.numel() else 1  # host bound: unreached action indices are not launched
        raw = self.engine.lookahead(self._cand_env, actions, n_act, max_n_actions=kmax)
        r, self.loop_clo = normalise_rewards(raw, self._cand_env.long(), self._cand_first, self.n_envs, self._graph["n_frontier"])
        return (r, raw) if return_raw else r

    # ------------------------------------------------------------------ step (exploration_env.py:98-105)
    def step(self, choice, check=True):
        """Execute, for every env, the plan of its chosen candidate. `choice` [n_envs] = frontier index within the env
        (int tensor / array) — `all_actions[key_size + action_index]` of policy.py:120.  A host array costs no synchronisation
        (the plans' lengths are on the host since actions_all_goals); check=False leaves the status check to the caller's next
        `engine.fetch` / `engine.check_status` (the trainers read the step's results with one)."""
        kmax = None
        if not torch.is_tensor(choice) and self._n_act_h is not None:
            c_h = self._cand_first_h + np.asarray(choice, dtype=np.int64)
            kmax = int(self._n_act_h[c_h].max())
            c = torch.as_tensor(c_h, device=self.device)
        else:
            c = self._cand_first + torch.as_tensor(choice, device=self.device).long()
        self.last_pick = c  # the chosen candidates' indices (device, int64)
        acts = self._actions[c]  # [n_envs, A, 3]
        nact = self._n_act[c]
        return self.step_actions(acts, nact, kmax=kmax, check=check)

    def step_actions(self, acts, nact, map_every_action=False, kmax=None, check=True):
        """Execute `nact[i]` actions of `acts[i]` in every env.  The virtual map is a pure function of the SLAM state, so it
        is rebuilt at each env's last action only unless `map_every_action` (per-step metrics of the map) asks otherwise.
        kmax: a host bound of nact (None: read from the device)."""
        if kmax is None:
            kmax = int(nact.max().item())
        if acts.shape[1] < self.cfg.max_actions:  # drlgx_step_plan strides the plans by the engine's max_actions
            acts = torch.cat([acts, acts.new_zeros(acts.shape[0], self.cfg.max_actions - acts.shape[1], 3)], dim=1)
        acts = acts.contiguous()
        nact = nact.to(torch.int32).contiguous()
        self.engine.step_plans(acts, nact, kmax, map_last_only=not map_every_action)
        live = torch.arange(acts.shape[1], device=self.device)[None, :] < nact[:, None]
        self.dist += (torch.sqrt(acts[:, :, 0] ** 2 + acts[:, :, 1] ** 2) * live).sum(dim=1)
        if check:
            self.engine.check_status()
        self._graph = None
        return self._get_obs(), self.done(), {}

    def step_traced(self, acts, nact, kmax=None, sigma0=1.0):
        """Execute `nact[i]` actions of `acts[i]` in every env the way the reference's evaluation loop does
        (scripts/test.py:128-152, Engine.step_plans_traced): the metrics of every executed action are recorded and an env leaves
        its plan behind the action at which done() holds (`explored > 0.85 or step > max_steps`), all on the device.  Returns
        device tensors (trace [n_envs, max_actions, 4], n_executed [n_envs] i32, done [n_envs] i32) and no synchronisation: the
        caller reads them - and the status word - with one `engine.fetch`.  kmax: a host bound of nact (None: read from the device)."""
        if kmax is None:
            kmax = int(nact.max().item()) if nact.numel() else 0
        if acts.shape[1] < self.cfg.max_actions:  # drlgx_step_plan strides the plans by the engine's max_actions
            acts = torch.cat([acts, acts.new_zeros(acts.shape[0], self.cfg.max_actions - acts.shape[1], 3)], dim=1)
        acts = acts.contiguous()
        trace, n_exec, done = self.engine.step_plans_traced(acts, nact, min(int(kmax), self.cfg.max_actions), sigma0=sigma0,
                                                            done_explored=0.85, max_steps=self._max_steps)
        live = torch.arange(acts.shape[1], device=self.device)[None, :] < n_exec[:, None]  # the EXECUTED actions only
        self.dist += (torch.sqrt(acts[:, :, 0] ** 2 + acts[:, :, 1] ** 2) * live).sum(dim=1)
        self._graph = None
        return trace, n_exec, done

    def follow(self, plan, n_actions, result, steps=5, active=None, sigma0=1.0):
        """Every env follows its plan the way the reference's explore() loop does (scripts/envs/pyplanner2d.py:100-109,170-187,
        Engine.follow_plans): `result` (em_plan's) selects the first min(steps, n_actions) edges, the fallback turn (0, 0, pi/4) of a
        SAMPLING_FAILURE, or nothing; an env stops behind the action at which done() holds or the obstacle flag is raised
        (Engine.set_env_obstacles) and in front of a rejected odometry, all on the device.  Returns device tensors (trace
        [n_envs, max_actions, 4], n_executed, done, stop [n_envs] i32 - Engine.STOP_*) and no synchronisation: the caller reads
        them - and the status word - with one `engine.fetch`.  self.dist advances by the executed actions' lengths."""
        A = self.cfg.max_actions
        if plan.shape[1] < A:
            plan = torch.cat([plan, plan.new_zeros(plan.shape[0], A - plan.shape[1], 3)], dim=1)
        plan = plan.contiguous()
        trace, n_exec, done, stop = self.engine.follow_plans(plan, n_actions, result, steps=steps, active=active, sigma0=sigma0,
                                                             done_explored=0.85, max_steps=self._max_steps)
        # (a fallback move has no length: only the plan's executed rows count, and those only for an env whose plan was followed)
        live = (torch.arange(A, device=self.device)[None, :] < n_exec[:, None]) & (result.to(self.device) == 3)[:, None]
        self.dist += (torch.sqrt(plan[:, :, 0] ** 2 + plan[:, :, 1] ** 2) * live).sum(dim=1)
        self._graph = None
        return trace, n_exec, done, stop

    def status(self):
        return self.engine.explored()

    def done(self):
        """exploration_env.py:107-110: `_done or step > max_steps or status() > 0.85` - the reference's terminal
        condition and nothing else."""
        c = self.engine.counts_dev()
        return (self.status() > 0.85) | (c[:, 3] > self._max_steps)

    def truncated(self):
        """Engine-side condition with no counterpart in the reference: envs whose trajectory is within one plan
        (max_actions poses) of the pose capacity.  Callers reset them WITHOUT treating the transition as terminal
        (the reference's episodes end on `explored > 0.85` only); with the default capacity of 256 poses this does not
        occur on the reference's maps."""
        c = self.engine.counts_dev()
        return c[:, 0] + self.cfg.max_actions + 1 > self.cfg.max_poses

    # ------------------------------------------------------------------ reporting
    def metrics(self, sigma0=1.0):
        """[n_envs, 3] float64 device tensor: get_landmark_error(), scripts/test.py's map_entropy(obs) and
        max_uncertainty_of_trajectory() of every env (scripts/test.py:136-142), computed on the device."""
        return self.engine.metrics(sigma0)

    # (host, one env)
    def get_landmark_size(self, i):
        return self.engine.counts(int(i))["landmarks"]

    def get_landmark_error(self, i, sigma0=1.0):
        """exploration_env.py:170-177."""
        keys, xy, _ = self.engine.landmarks(int(i))
        _, gt = self.engine.ground_truth(int(i))
        err = float(np.sqrt(((gt[keys] - xy) ** 2).sum(axis=1)).sum()) if len(keys) else 0.0
        n_gt = self.cfg.num_landmarks
        return (err + sigma0 * (n_gt - len(keys))) / n_gt

    def max_uncertainty_of_trajectory(self, i):
        """exploration_env.py:190-194."""
        _, X = self.engine.adjacency(int(i))
        return float(np.amax(X[self.get_landmark_size(i):]))
