"""Thin object wrapper over the C ABI (include/drlgx.h): one `Engine` = one drlgx_engine handle.

Bulk inputs/outputs are torch CUDA tensors (torch is used only for device memory and streams); the
`*_host` getters return numpy arrays and mirror the getters of the reference's pybind modules.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .config import DrlgxConfig, start_pose


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8,
          torch.bool: np.bool_, torch.int16: np.int16, torch.int8: np.int8}


class Engine(object):
    def __init__(self, cfg, n_envs, n_rollouts=0, device=0):
        if not isinstance(cfg, DrlgxConfig):
            raise TypeError("cfg must be a DrlgxConfig")
        if not torch.cuda.is_available():
            raise _lib.DrlgxError("no HIP device visible: the drlgx engine has no CPU fallback")
        self.L = _lib.lib()
        self.cfg = cfg
        self.n_envs = n_envs
        self.n_rollouts = n_rollouts
        self.device = torch.device("cuda", device)
        self.h = C.c_void_p()
        self.sampler_parameter, self.sampler_obstacles = (0.5, 0.0, False), False  # (the engine's values after drlgx_create)
        self.dubins_parameter = None
        self.dubins_leaf_scoring = False
        self.env_obstacles = False
        _lib.check(self.L.drlgx_create(C.byref(cfg), n_envs, n_rollouts, device, C.byref(self.h)), self.h)  # (NULL: the creation's error)
        r, c = C.c_int32(), C.c_int32()
        self.L.drlgx_vm_shape(self.h, C.byref(r), C.byref(c))
        self.rows, self.cols = r.value, c.value
        self.use_torch_stream()

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.drlgx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        _lib.check(rc, self.h)

    def use_torch_stream(self):
        """Enqueue engine kernels on torch's current stream of the engine's device, so that tensors can be shared
        without syncs.  Called before every call that enqueues work (cheap when the stream has not changed), so the
        engine follows `with torch.cuda.stream(...)` blocks."""
        s = _lib.stream_ptr(self.device)
        if s != getattr(self, "_bound_stream", None):
            self._chk(self.L.drlgx_set_stream(self.h, C.c_void_p(s)))
            self._bound_stream = s

    def synchronize(self):
        self._chk(self.L.drlgx_synchronize(self.h))

    def status(self):
        return self.L.drlgx_status_host(self.h)

    def check_status(self):
        st = self.status()
        if st != 0:
            _lib.check(st, self.h)

    def fetch(self, *tensors):
        """check_status() with the given device tensors brought to the host under the same synchronisation (one stream drain and
        one copy instead of a `.cpu()` / `.item()` each): returns one numpy array per tensor, same dtype and shape."""
        self.use_torch_stream()
        for t in tensors:
            if t.device != self.device:
                raise ValueError("Engine.fetch reads tensors on the engine's device (%s), not %s" % (self.device, t.device))
        parts = [t.detach().contiguous().view(-1).view(torch.uint8) for t in tensors]
        n = sum(p.numel() for p in parts)
        if n == 0:
            self.check_status()
            return [np.empty(tuple(t.shape), dtype=_NP_OF[t.dtype]) for t in tensors]
        packed = parts[0] if len(parts) == 1 else torch.cat(parts)
        host = getattr(self, "_fetch_host", None)
        if host is None or host.numel() < n:
            host = self._fetch_host = torch.empty(max(2 * n, 1 << 16), dtype=torch.uint8, pin_memory=True)
        st = self.L.drlgx_status_fetch_host(self.h, _p(packed), n, C.c_void_p(host.data_ptr()))
        if st != 0:
            _lib.check(st, self.h)
        raw = host.numpy()
        out, off = [], 0
        for t, p in zip(tensors, parts):
            k = p.numel()
            out.append(raw[off:off + k].copy().view(_NP_OF[t.dtype]).reshape(tuple(t.shape)))
            off += k
        return out

    # ---- life cycle
    def reset(self, env_ids, seeds, starts=None, los=None):
        """SS2D.__init__ for the listed envs. starts: (n,3) x,y,theta; or `los` to use the reference's
        legacy numpy start-pose stream (pyss2d.py:89-95)."""
        self.use_torch_stream()
        env_ids = np.ascontiguousarray(env_ids, dtype=np.int32)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        if starts is None:
            starts = np.array([start_pose(int(lo), self.cfg.map_max_x) for lo in los], dtype=np.float64)
        starts = np.ascontiguousarray(starts, dtype=np.float64)
        self._chk(self.L.drlgx_reset_host(self.h, len(env_ids), env_ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                          seeds.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          starts.ctypes.data_as(C.POINTER(C.c_double))))

    def step(self, odom, active=None):
        """SS2D.simulate(core=True) for all envs. odom: CUDA float64 [n_envs,3]; active: CUDA uint8 [n_envs]."""
        self.use_torch_stream()
        assert odom.is_cuda and odom.dtype == torch.float64 and odom.is_contiguous()
        self._chk(self.L.drlgx_step(self.h, _p(odom), _p(active)))

    # ---- staged belief step (one call per call of the reference's SS2D.__init__ / SS2D.simulate)

    def step_plan(self, actions, n_actions, action_index, map_last_only=True):
        """One action index of every env's plan (drlgx_step_plan): actions [n_envs, max_actions, 3] f64, n_actions [n_envs]
        i32 on the device; with `map_last_only` the virtual map is rebuilt at each env's last action only."""
        self.use_torch_stream()
        self._chk(self.L.drlgx_step_plan(self.h, _p(actions), _p(n_actions), int(action_index), 1 if map_last_only else 0))

    def step_plans(self, actions, n_actions, max_n_actions, map_last_only=True):
        """Every env's whole plan (drlgx_step_plans): `for k in range(max_n_actions): step_plan(..., k)` in one call."""
        self.use_torch_stream()
        self._chk(self.L.drlgx_step_plans(self.h, _p(actions), _p(n_actions), int(max_n_actions), 1 if map_last_only else 0))

    def step_plans_traced(self, actions, n_actions, max_n_actions, sigma0=1.0, done_explored=0.85, max_steps=5000):
        """Every env's plan as the reference's evaluation loop executes it (drlgx_step_plans_traced, scripts/test.py:128-152): per
        executed action the row (landmark error, map entropy, max localisation uncertainty, explored), and an env stops behind
        the action at which `explored > done_explored or step > max_steps` holds - on the device.  Returns device tensors
        (trace [n_envs, max_actions, 4] f64, pre-filled with NaN: rows beyond an env's executed actions keep it; n_executed
        [n_envs] i32; done [n_envs] i32).  `n_actions` is left as it is."""
        self.use_torch_stream()
        A = self.cfg.max_actions
        if not (actions.is_cuda and actions.dtype == torch.float64 and actions.is_contiguous() and
                tuple(actions.shape) == (self.n_envs, A, 3)):
            raise ValueError("actions: contiguous CUDA float64 [n_envs, max_actions, 3]")
        n_exec = n_actions.to(torch.int32).clamp(0, A).contiguous().clone()
        if n_exec.numel() != self.n_envs:
            raise ValueError("n_actions: [n_envs]")
        trace = torch.full((self.n_envs, A, 4), float("nan"), dtype=torch.float64, device=self.device)
        done = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self._chk(self.L.drlgx_step_plans_traced(self.h, _p(actions), _p(n_exec), int(max_n_actions), float(sigma0),
                                                 float(done_explored), int(max_steps), _p(trace), _p(done)))
        return trace, n_exec, done

    def set_env_obstacles(self, enabled):
        """SS2D.simulate's obstacle flag at cfg.safe_distance > 0 (drlgx_set_env_obstacles): an opt-in, off after creation - the ini
        files' [Environment] safe_distance is otherwise inert.  The beliefs do not change; every step also leaves obstacle_flags()."""
        self._chk(self.L.drlgx_set_env_obstacles(self.h, 1 if enabled else 0))
        self.env_obstacles = bool(enabled)

    def obstacle_flags(self):
        """(obstacle [n_envs] uint8: the last step's flag, cleared [n_envs] uint8: the latch) on the device (drlgx_obstacle_flags)."""
        self.use_torch_stream()
        out = torch.empty(2, self.n_envs, dtype=torch.uint8, device=self.device)
        self._chk(self.L.drlgx_obstacle_flags(self.h, _p(out)))
        return out[0], out[1]

    STOP_RAN, STOP_DONE, STOP_OBSTACLE, STOP_REJECTED, STOP_NO_SOLUTION, STOP_TERMINATION = range(6)

    def follow_plans(self, plan, n_actions, result, steps=5, active=None, fallback=(0.0, 0.0, math.pi / 4), sigma0=1.0, done_explored=0.85,
                     max_steps=5000):
        """Every env follows its plan as EMExplorer.follow_path / explore() do (drlgx_follow_plans, pyplanner2d.py:100-109,170-187):
        SUCCESS (3) the first min(steps, n_actions) rows, SAMPLING_FAILURE (0) the fallback move, NO_SOLUTION / TERMINATION or an
        inactive env nothing; an env stops behind a step that is done or raises the obstacle flag (set_env_obstacles) and in front
        of a rejected odometry - on the device.  Returns device tensors (trace [n_envs, max_actions, 4] f64, NaN beyond the
        executed actions; n_executed, done, stop [n_envs] i32 - stop: the STOP_* codes)."""
        self.use_torch_stream()
        A = self.cfg.max_actions
        if not (plan.is_cuda and plan.dtype == torch.float64 and plan.is_contiguous() and tuple(plan.shape) == (self.n_envs, A, 3)):
            raise ValueError("plan: contiguous CUDA float64 [n_envs, max_actions, 3]")
        n_actions = n_actions.to(torch.int32).contiguous()
        result = result.to(torch.int32).contiguous()
        if n_actions.numel() != self.n_envs or result.numel() != self.n_envs:
            raise ValueError("n_actions, result: [n_envs]")
        if active is not None:
            active = active.to(torch.uint8).contiguous()
        trace = torch.full((self.n_envs, A, 4), float("nan"), dtype=torch.float64, device=self.device)
        n_exec = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        done = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        stop = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        fb = (C.c_double * 3)(*[float(v) for v in fallback])
        self._chk(self.L.drlgx_follow_plans(self.h, _p(plan), _p(n_actions), _p(result), _p(active), int(steps), fb, float(sigma0),
                                            float(done_explored), int(max_steps), _p(trace), _p(n_exec), _p(done), _p(stop)))
        return trace, n_exec, done, stop

    @staticmethod
    def greedy_plans(score, seg_begin, n_frontier, actions_pad, n_act_pad, active=None):
        """The greedy decision of every env on the device (drlgx_greedy_plans; stateless - it runs on torch's current stream of the
        tensors' device and needs no engine handle): the first arg-max of `score` (f32) over the env's
        frontier segment [seg_begin[e], + n_frontier[e]) in numpy's order (a NaN first) and that frontier's plan out of
        `graph(plan=True)`'s actions_pad [n_envs, Fmax, A, 3] / n_act_pad [n_envs, Fmax].  Returns (choice [n_envs] i32, -1 for
        an inactive env or one without frontiers; actions [n_envs, A, 3] f64, zero behind the plan; n_actions [n_envs] i32)."""
        n, mf, A = actions_pad.shape[0], actions_pad.shape[1], actions_pad.shape[2]
        dev = actions_pad.device
        if score.dtype != torch.float32 or actions_pad.dtype != torch.float64 or n_act_pad.dtype != torch.int32:
            raise ValueError("score float32, actions_pad float64, n_act_pad int32")
        if tuple(n_act_pad.shape) != (n, mf) or seg_begin.numel() != n or n_frontier.numel() != n:
            raise ValueError("greedy_plans: shapes disagree")
        score, actions_pad, n_act_pad = score.contiguous(), actions_pad.contiguous(), n_act_pad.contiguous()
        seg_begin, n_frontier = seg_begin.to(torch.int32).contiguous(), n_frontier.to(torch.int32).contiguous()
        if active is not None:
            active = active.to(torch.uint8).contiguous()
        choice = torch.empty(n, dtype=torch.int32, device=dev)
        acts = torch.empty(n, A, 3, dtype=torch.float64, device=dev)
        n_act = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().drlgx_greedy_plans(C.c_void_p(_lib.stream_ptr(dev)), n, _p(score), score.numel(), _p(seg_begin), _p(n_frontier), _p(active),
                                             _p(actions_pad), _p(n_act_pad), mf, A, _p(choice), _p(acts), _p(n_act)))
        return choice, acts, n_act

    def stage_reset(self, env_ids, seeds, starts):
        env_ids = np.ascontiguousarray(env_ids, dtype=np.int32)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        starts = np.ascontiguousarray(starts, dtype=np.float64)
        self.use_torch_stream()
        self._chk(self.L.drlgx_stage_reset_host(self.h, len(env_ids), env_ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                seeds.ctypes.data_as(C.POINTER(C.c_uint32)), starts.ctypes.data_as(C.POINTER(C.c_double))))

    def stage_set_prior_information(self, env, information):
        """A full 3 x 3 prior information for one env (after stage_reset, before the first optimise)."""
        info = np.ascontiguousarray(information, dtype=np.float64).reshape(9)
        self._chk(self.L.drlgx_stage_set_prior_information_host(self.h, int(env), info.ctypes.data_as(C.POINTER(C.c_double))))

    def stage_set_prior_pose(self, env, xytheta):
        """The pose of the prior factor / the initial estimate of x0 for one env (after stage_reset, before the first measurement)."""
        p = np.ascontiguousarray(xytheta, dtype=np.float64).reshape(3)
        self._chk(self.L.drlgx_stage_set_prior_pose_host(self.h, int(env), p.ctypes.data_as(C.POINTER(C.c_double))))

    def stage_move(self, odom, active=None):
        self.use_torch_stream()
        self._chk(self.L.drlgx_stage_move(self.h, _p(odom), _p(active)))

    def stage_measure(self, active=None):
        """One Simulator2D::measure per env: (keys [n, LG] i32, bearing_range [n, LG, 2] f64, count [n] i32)."""
        self.use_torch_stream()
        lg = max(self.cfg.num_landmarks, 1)
        keys = torch.zeros(self.n_envs, lg, dtype=torch.int32, device=self.device)
        br = torch.zeros(self.n_envs, lg, 2, dtype=torch.float64, device=self.device)
        cnt = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self._chk(self.L.drlgx_stage_measure(self.h, _p(active), _p(keys), _p(br), _p(cnt)))
        return keys, br, cnt

    def stage_add_measurements(self, keys, br, cnt, active=None):
        self.use_torch_stream()
        self._chk(self.L.drlgx_stage_add_measurements(self.h, _p(active), _p(keys), _p(br), _p(cnt)))

    def stage_optimize(self, active=None):
        self.use_torch_stream()
        self._chk(self.L.drlgx_stage_optimize(self.h, _p(active)))

    def stage_update_map(self, active=None, rebuild=True):
        self.use_torch_stream()
        self._chk(self.L.drlgx_stage_update_map(self.h, _p(active), int(bool(rebuild))))

    def set_fixed_landmarks(self, xy):
        """The listed ground-truth landmarks of `Simulator2D.random_landmarks(landmarks, num, params)` (keys 0 .. k - 1 of every
        env; cfg.num_landmarks is the total): effective at the next reset."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._chk(self.L.drlgx_set_fixed_landmarks_host(self.h, len(xy), xy.ctypes.data_as(C.POINTER(C.c_double))))

    def set_planner_parameter(self, angle_weight, distance_weight0, distance_weight1, occupancy_threshold, max_edge_length, algorithm):
        self._chk(self.L.drlgx_set_planner_parameter(self.h, float(angle_weight), float(distance_weight0), float(distance_weight1),
                                                     float(occupancy_threshold), float(max_edge_length), int(algorithm)))
        for k, v in (("angle_weight", angle_weight), ("distance_weight0", distance_weight0), ("distance_weight1", distance_weight1),
                     ("occupancy_threshold", occupancy_threshold), ("max_edge_length", max_edge_length), ("algorithm", int(algorithm))):
            setattr(self.cfg, k, v)

    def _core_mask(self, core, n):
        if core.dtype != torch.uint8 or tuple(core.shape) != (n, self.cfg.max_actions) or not core.is_contiguous():
            raise ValueError("core: a contiguous uint8 tensor [C, max_actions] expected")
        return core

    def fm2_update(self, cand_env, actions, n_actions, core=None):
        """FastMarginals2-style covariance look-ahead (drlgx_fm2_update): returns (cov [C, max_poses + max_actions, 3, 3]
        float64, n_poses [C] int32); rows beyond n_poses[c] are undefined.  `core` (uint8 [C, max_actions] on the device, or None =
        every action): the actions that are core poses - a non-core step extends the chain and predicts no measurement
        (drlgx_fm2_update_steps)."""
        self.use_torch_stream()
        n = cand_env.numel()
        stride = self.cfg.max_poses + self.cfg.max_actions
        cov = torch.zeros(n, stride, 3, 3, dtype=torch.float64, device=self.device)
        n_out = torch.zeros(n, dtype=torch.int32, device=self.device)
        if core is None:
            self._chk(self.L.drlgx_fm2_update(self.h, n, _p(cand_env), _p(actions), _p(n_actions), _p(cov), stride, _p(n_out)))
        else:
            self._chk(self.L.drlgx_fm2_update_steps(self.h, n, _p(cand_env), _p(actions), _p(n_actions), _p(self._core_mask(core, n)),
                                                    _p(cov), stride, _p(n_out)))
        return cov, n_out

    def em_cost(self, cand_env, actions, n_actions, algorithm=0, want_info=False, core=None, distance=None):
        """Expected look-ahead cost of candidate plans (drlgx_em_cost: the leaf evaluation of EMPlanner2D::optimize2, without
        simulating or re-solving): returns (uncertainty [C], cost [C]) float64 and, with `want_info`, the leaf virtual map's
        information [C, rows, cols, 3] (xx, xy, yy).  cand_env [C] i32, actions [C, max_actions, 3] f64, n_actions [C] i32 on the
        device; algorithm 0 = EM_AOPT, 1 = EM_DOPT.  `core` (uint8 [C, max_actions]) / `distance` (f64 [C]), device tensors or
        None: the leaves of a tree with non-core steps (drlgx_em_cost_steps) - only core poses predict measurements and enter the
        leaf's map, the cost takes `distance` instead of the plan's own."""
        self.use_torch_stream()
        n = cand_env.numel()
        unc = torch.empty(n, dtype=torch.float64, device=self.device)
        cost = torch.empty(n, dtype=torch.float64, device=self.device)
        info = torch.empty(n, self.rows, self.cols, 3, dtype=torch.float64, device=self.device) if want_info else None
        if core is None and distance is None:
            self._chk(self.L.drlgx_em_cost(self.h, n, _p(cand_env), _p(actions), _p(n_actions), int(algorithm), _p(unc), _p(cost), _p(info)))
        else:
            if core is not None:
                core = self._core_mask(core, n)
            if distance is not None and (distance.dtype != torch.float64 or distance.numel() != n or not distance.is_contiguous()):
                raise ValueError("distance: a contiguous float64 tensor [C] expected")
            self._chk(self.L.drlgx_em_cost_steps(self.h, n, _p(cand_env), _p(actions), _p(n_actions), _p(core), _p(distance),
                                                 int(algorithm), _p(unc), _p(cost), _p(info)))
        return (unc, cost, info) if want_info else (unc, cost)

    def og_cost(self, cand_env, actions, n_actions, want_prob=False):
        """Expected map entropy of candidate plans (drlgx_og_cost: calculateUncertainty_OG_SHANNON and costFunction, without
        simulating, re-solving or any covariance): returns (entropy [C], cost [C]) float64 and, with `want_prob`, the leaf
        occupancy map's probabilities [C, rows, cols].  Candidates as in `em_cost`: cand_env [C] i32, actions
        [C, max_actions, 3] f64, n_actions [C] i32 on the device."""
        self.use_torch_stream()
        n = cand_env.numel()
        ent = torch.empty(n, dtype=torch.float64, device=self.device)
        cost = torch.empty(n, dtype=torch.float64, device=self.device)
        prob = torch.empty(n, self.rows, self.cols, dtype=torch.float64, device=self.device) if want_prob else None
        self._chk(self.L.drlgx_og_cost(self.h, n, _p(cand_env), _p(actions), _p(n_actions), _p(ent), _p(cost), _p(prob)))
        return (ent, cost, prob) if want_prob else (ent, cost)

    def slam_og_cost(self, cand_env, actions, n_actions, alpha, core=None, distance=None, want_terms=False, want_lm_cov=False):
        """SLAM-OG-Shannon cost of candidate plans (drlgx_slam_og_cost: calculateUncertainty_SLAM_OG_SHANNON and costFunction,
        without simulating or re-solving): the expected map entropy of `og_cost` weighed against the landmarks' uncertainty after the
        covariance update of `fm2_update` - uncertainty = w2 H_leaf + w1 sum_l sqrt(det Sigma'(l, l)), w2 = (1 - alpha) / H_root and
        w1 = alpha / sum_l sqrt(det cov_l) from the live belief (an environment without a landmark has w1 = inf and NaN
        uncertainties, as the reference's plain divisions give).  Returns (uncertainty [C], cost [C]) float64 and, with
        `want_terms`, terms [C, 2] (H_leaf, slam_uncertainty) and weights [n_envs, 2] (w1, w2); with `want_lm_cov` the landmarks'
        updated blocks [C, max_landmarks, 3] (xx, xy, yy per slot; rows beyond the environment's landmark count are NaN).
        Candidates as in `em_cost`: cand_env [C] i32, actions [C, max_actions, 3] f64, n_actions [C] i32 on the device, C >= 1;
        alpha in [0, 1]; `core` (uint8 [C, max_actions]) / `distance` (f64 [C]), device tensors or None, as `em_cost`'s."""
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError("alpha must lie in [0, 1], not %r" % (alpha,))
        self.use_torch_stream()
        n = cand_env.numel()
        if core is not None:
            core = self._core_mask(core, n)
        if distance is not None and (distance.dtype != torch.float64 or distance.numel() != n or not distance.is_contiguous()):
            raise ValueError("distance: a contiguous float64 tensor [C] expected")
        unc = torch.empty(n, dtype=torch.float64, device=self.device)
        cost = torch.empty(n, dtype=torch.float64, device=self.device)
        terms = torch.empty(n, 2, dtype=torch.float64, device=self.device) if want_terms else None
        weights = torch.empty(self.n_envs, 2, dtype=torch.float64, device=self.device) if want_terms else None
        lm_cov = torch.full((n, self.cfg.max_landmarks, 3), float("nan"), dtype=torch.float64, device=self.device) if want_lm_cov else None
        self._chk(self.L.drlgx_slam_og_cost(self.h, n, _p(cand_env), _p(actions), _p(n_actions), _p(core), _p(distance), float(alpha),
                                            _p(unc), _p(cost), _p(terms), _p(weights), _p(lm_cov)))
        out = (unc, cost)
        if want_terms:
            out += (terms, weights)
        if want_lm_cov:
            out += (lm_cov,)
        return out

    def set_sampler_parameter(self, max_nodes, safe_distance=0.0, dubins_control_model_enabled=False):
        """The planner parameters only the tree sampler reads (drlgx_set_sampler_parameter); a non-zero safe_distance or the Dubins
        control model is stored and then refused by em_plan / rrt_plan (a safe_distance >= 0 is served once
        set_sampler_obstacles(True) has opted in; the Dubins control model is served by rrt_plan once set_dubins_library has loaded
        a library, and by em_plan once set_dubins_leaf_scoring(True) has opted in as well).  The values last set are kept in `sampler_parameter`."""
        self._chk(self.L.drlgx_set_sampler_parameter(self.h, float(max_nodes), float(safe_distance), int(bool(dubins_control_model_enabled))))
        self.sampler_parameter = (float(max_nodes), float(safe_distance), bool(dubins_control_model_enabled))

    def set_sampler_obstacles(self, enabled):
        """The sampler's obstacle logic (drlgx_set_sampler_obstacles), an opt-in that is off after construction: with it em_plan /
        rrt_plan serve safe_distance >= 0 - isSafe on samples and edges, the retry loop of sampleNode, the two counters of 1000 and
        the shrink at the start of a call, as the reference has them; a tree can then end with SAMPLING_FAILURE (a result, not an
        error).  Off, a non-zero safe_distance is refused as before.  The setting is kept in `sampler_obstacles`."""
        self._chk(self.L.drlgx_set_sampler_obstacles(self.h, int(bool(enabled))))
        self.sampler_obstacles = bool(enabled)

    def set_dubins_leaf_scoring(self, enabled):
        """em_plan under the Dubins control model (drlgx_set_dubins_leaf_scoring), an opt-in that is off after construction: with
        it, a library loaded and the sampler's Dubins flag set, em_plan grows the Dubins tree with optimize2's stop rule and scores
        every leaf with its non-core steps (one plan row per step, the core mask 1 at each edge's last step, the tree's distance).
        Off, em_plan under the Dubins flag is refused as before.  The setting is kept in `dubins_leaf_scoring`."""
        self._chk(self.L.drlgx_set_dubins_leaf_scoring(self.h, int(bool(enabled))))
        self.dubins_leaf_scoring = bool(enabled)

    def em_plan_leaves(self):
        """The leaves the last served em_plan or og_plan scored (drlgx_em_plan_leaves), in candidate order: a dict of device tensors cand_env
        [C] i32, actions [C, max_actions, 3] f64, n_actions [C] i32, core [C, max_actions] u8, cost [C] f64 and, when that call ran
        the Dubins control model (whatever the sampler's flag says now), distance [C] f64 (else None)."""
        self.use_torch_stream()
        n, steps = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.drlgx_em_plan_leaves(self.h, 0, C.byref(n), C.byref(steps), None, None, None, None, None, None))
        c, A, dev = int(n.value), self.cfg.max_actions, self.device
        o = dict(cand_env=torch.empty(c, dtype=torch.int32, device=dev), actions=torch.empty(c, A, 3, dtype=torch.float64, device=dev),
                 n_actions=torch.empty(c, dtype=torch.int32, device=dev), core=torch.empty(c, A, dtype=torch.uint8, device=dev),
                 cost=torch.empty(c, dtype=torch.float64, device=dev), distance=None)
        if steps.value:
            o["distance"] = torch.empty(c, dtype=torch.float64, device=dev)
        self._chk(self.L.drlgx_em_plan_leaves(self.h, c, C.byref(n), None, _p(o["cand_env"]), _p(o["actions"]), _p(o["n_actions"]), _p(o["core"]),
                                              _p(o["distance"]), _p(o["cost"])))
        return o

    DUBINS_FIELDS = ("max_w", "dw", "min_v", "max_v", "dv", "dt", "min_duration", "max_duration", "tolerance_radius")

    def set_dubins_library(self, parameter):
        """The Dubins path library (drlgx_set_dubins_library_host), and with it the opt-in of the Dubins control model: `parameter`
        is a planner2d.DubinsParameter (or any object / sequence with its nine fields in DUBINS_FIELDS order); None clears the
        library.  The engine builds the library with the reference's loops; with one loaded and the Dubins flag of
        set_sampler_parameter set, rrt_plan is served (one plan row per step, nodes columns 5-7 = library index, num_steps, 0);
        em_plan stays refused unless set_dubins_leaf_scoring(True) has opted in.  Raises DrlgxError for parameters the engine refuses.  Returns the library's size."""
        self.dubins_parameter = None  # (the nine values of the library loaded last, for callers that would load it again)
        if parameter is None:
            self._chk(self.L.drlgx_set_dubins_library_host(self.h, None))
            return 0
        vals = [float(getattr(parameter, f)) for f in self.DUBINS_FIELDS] if hasattr(parameter, "max_w") else [float(x) for x in parameter]
        if len(vals) != 9:
            raise ValueError("nine Dubins parameters expected: %s" % ", ".join(self.DUBINS_FIELDS))
        arr = (C.c_double * 9)(*vals)
        self._chk(self.L.drlgx_set_dubins_library_host(self.h, arr))
        self.dubins_parameter = tuple(vals)
        return self.dubins_library_size()

    def dubins_library_size(self):
        n = C.c_int32(0)
        self._chk(self.L.drlgx_dubins_library(self.h, 0, C.byref(n), None, None, None, None))
        return int(n.value)

    def dubins_library(self):
        """The library as the engine built it (drlgx_dubins_library), in library order: a dict of numpy arrays end [n, 3] (x, y,
        theta), v, w [n] f64, num_steps [n] i32; n = 0 with no library loaded."""
        n = self.dubins_library_size()
        end, v, w = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
        steps = np.zeros(n, dtype=np.int32)
        got = C.c_int32(0)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self._chk(self.L.drlgx_dubins_library(self.h, n, C.byref(got), end.ctypes.data_as(dp), v.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                              steps.ctypes.data_as(ip)))
        return dict(end=end, v=v, w=w, num_steps=steps)

    def set_dubins_prefilter(self, enabled):
        """The library scan's exact pre-filter (drlgx_set_dubins_prefilter; on after construction): off, every sample scans the
        library; the results are the same."""
        self._chk(self.L.drlgx_set_dubins_prefilter(self.h, int(bool(enabled))))

    def _tree_outputs(self, n, max_tree_nodes, want_nodes):
        dev, A = self.device, self.cfg.max_actions
        out = dict(plan=torch.empty(n, A, 3, dtype=torch.float64, device=dev),
                   n_actions=torch.empty(n, dtype=torch.int32, device=dev),
                   result=torch.empty(n, dtype=torch.int32, device=dev),
                   halton_next=torch.empty(n, dtype=torch.int32, device=dev),
                   n_nodes=torch.empty(n, dtype=torch.int32, device=dev),
                   nodes=torch.zeros(n, int(max_tree_nodes), 8, dtype=torch.float64, device=dev) if want_nodes else None)
        return out

    def em_plan(self, env_sel, halton_start, max_tree_nodes=1024, algorithm=0, want_nodes=False):
        """EMPlanner2D::optimize2 for the listed environments (drlgx_em_plan): one tree per environment grown on the device from
        Halton point `halton_start[i]` on, its leaves scored by the body of em_cost, the first leaf with the strictly smallest cost
        taken.  env_sel, halton_start [n] i32 on the device.  Returns a dict of device tensors: plan [n, max_actions, 3] f64 (edge
        odometry root -> leaf), n_actions, result (OptimizationResult), n_leaves, halton_next, n_nodes [n] i32, cost [n] f64 and,
        with `want_nodes`, nodes [n, max_tree_nodes, 8] f64 (x y theta parent distance | edge odometry x y theta).  Raises
        DrlgxError on a refusal (capacity: a tree beyond max_tree_nodes or deeper than cfg.max_actions).  Under the Dubins control
        model (set_dubins_library, the sampler's Dubins flag and set_dubins_leaf_scoring(True)) the plan has one row per step, nodes
        columns 5-7 are (library index, num_steps, 0), and a tree can end with SAMPLING_FAILURE; em_plan_leaves() reads back what was
        scored."""
        self.use_torch_stream()
        n = env_sel.numel()
        o = self._tree_outputs(n, max_tree_nodes, want_nodes)
        o["cost"] = torch.empty(n, dtype=torch.float64, device=self.device)
        o["n_leaves"] = torch.empty(n, dtype=torch.int32, device=self.device)
        self._chk(self.L.drlgx_em_plan(self.h, n, _p(env_sel), _p(halton_start), int(max_tree_nodes), int(algorithm), _p(o["plan"]),
                                       _p(o["n_actions"]), _p(o["cost"]), _p(o["result"]), _p(o["n_leaves"]), _p(o["halton_next"]),
                                       _p(o["nodes"]), _p(o["n_nodes"])))
        return o

    def og_plan(self, env_sel, halton_start, max_tree_nodes=1024, algorithm=2, alpha=0.0, want_nodes=False):
        """EMPlanner2D::optimize2 under OG_SHANNON (algorithm 2) or SLAM_OG_SHANNON (algorithm 3) for the listed environments
        (drlgx_og_plan): em_plan's tree, leaves and pick, the leaves scored with the cost of `og_cost` or of `slam_og_cost(alpha)` -
        the same bits as those calls on the same leaves.  `alpha` (in [0, 1]) is read under algorithm 3 only.  Returns the dict of
        em_plan; em_plan_leaves() reads back what was scored.  The Dubins control model is refused."""
        self.use_torch_stream()
        n = env_sel.numel()
        o = self._tree_outputs(n, max_tree_nodes, want_nodes)
        o["cost"] = torch.empty(n, dtype=torch.float64, device=self.device)
        o["n_leaves"] = torch.empty(n, dtype=torch.int32, device=self.device)
        self._chk(self.L.drlgx_og_plan(self.h, n, _p(env_sel), _p(halton_start), int(max_tree_nodes), int(algorithm), float(alpha),
                                       _p(o["plan"]), _p(o["n_actions"]), _p(o["cost"]), _p(o["result"]), _p(o["n_leaves"]),
                                       _p(o["halton_next"]), _p(o["nodes"]), _p(o["n_nodes"])))
        return o

    def rrt_plan(self, env_sel, goal_key, goal_xy, halton_start, max_tree_nodes=1024, want_nodes=False):
        """EMPlanner2D::rrt_planner for the listed environments (drlgx_rrt_plan): the tree grown until a node lies within
        max_edge_length of the goal - graph node goal_key[i] if it is one (landmarks in key order, then poses), else the point
        goal_xy[i] -, the plan the path root -> goal.  A tree that fills max_tree_nodes first has result SAMPLING_FAILURE and
        no actions.  Returns the dict of em_plan without cost / n_leaves.  Under the Dubins control model (set_dubins_library and the
        sampler's Dubins flag) the plan has one row per step and nodes columns 5-7 are (library index, num_steps, 0)."""
        self.use_torch_stream()
        n = env_sel.numel()
        o = self._tree_outputs(n, max_tree_nodes, want_nodes)
        self._chk(self.L.drlgx_rrt_plan(self.h, n, _p(env_sel), _p(goal_key), _p(goal_xy), _p(halton_start), int(max_tree_nodes),
                                        _p(o["plan"]), _p(o["n_actions"]), _p(o["result"]), _p(o["halton_next"]), _p(o["nodes"]),
                                        _p(o["n_nodes"])))
        return o

    def utility(self, dist=None):
        self.use_torch_stream()
        out = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        self._chk(self.L.drlgx_utility(self.h, _p(dist), _p(out)))
        return out

    def uncertainty_em(self, algorithm):
        self.use_torch_stream()
        out = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        self._chk(self.L.drlgx_uncertainty_em(self.h, int(algorithm), _p(out)))
        return out

    def explored(self):
        self.use_torch_stream()
        out = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        self._chk(self.L.drlgx_explored(self.h, _p(out)))
        return out

    def metrics(self, sigma0=1.0):
        """[n_envs, 3] float64 CUDA tensor: landmark error, map entropy, max localisation uncertainty - the columns
        scripts/test.py:136-142 writes per executed action."""
        self.use_torch_stream()
        out = torch.empty(self.n_envs, 3, dtype=torch.float64, device=self.device)
        self._chk(self.L.drlgx_metrics(self.h, float(sigma0), _p(out)))
        return out

    def cov_array(self):
        """VirtualMap.to_cov_array for every env: (length, angle) [n_envs, rows, cols] float64 CUDA tensors."""
        self.use_torch_stream()
        ln = torch.empty(self.n_envs, self.rows, self.cols, dtype=torch.float64, device=self.device)
        an = torch.empty_like(ln)
        self._chk(self.L.drlgx_cov_array(self.h, _p(ln), _p(an)))
        return ln, an

    def line_plan(self, cand_env, goals):
        self.use_torch_stream()
        n = cand_env.numel()
        A = self.cfg.max_actions
        actions = torch.zeros(n, A, 3, dtype=torch.float64, device=self.device)
        n_act = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._chk(self.L.drlgx_line_plan(self.h, n, _p(cand_env), _p(goals), _p(actions), _p(n_act)))
        return actions, n_act

    def lookahead(self, cand_env, actions, n_actions, max_n_actions=None):
        """Look-ahead rewards; `max_n_actions` (host int >= every n_actions[i]) skips the launches of the action indices
        no plan reaches (None: all cfg.max_actions indices are launched)."""
        self.use_torch_stream()
        n = cand_env.numel()
        rewards = torch.empty(n, dtype=torch.float64, device=self.device)
        if max_n_actions is None:
            self._chk(self.L.drlgx_lookahead(self.h, n, _p(cand_env), _p(actions), _p(n_actions), _p(rewards)))
        else:
            self._chk(self.L.drlgx_lookahead_bounded(self.h, n, _p(cand_env), _p(actions), _p(n_actions), int(max_n_actions),
                                                     _p(rewards)))
        return rewards

    def graph_capacity(self):
        """(max nodes, max edges, max frontiers per env) of one batched export."""
        if not hasattr(self, "_gcap"):
            a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
            self._chk(self.L.drlgx_graph_capacity(self.h, C.byref(a), C.byref(b), C.byref(c)))
            self._gcap = (a.value, b.value, c.value)
        return self._gcap

    def graph(self, plan=False):
        """Batched ExplorationEnv.graph_matrix + DeepQ.data_process for all envs (one PyG-style batch).
        Returns a dict of CUDA tensors: x [N,5] f32, edge_index [2,E] i64, edge_attr [E] f32, node_off / edge_off
        [n_envs+1] i32, batch [N] i64, n_frontier [n_envs] i32, frontier_xy [n_envs,Fmax,2] f64,
        nearest_frontier_node [n_envs] i32 (local node id); max_graph_edges = the largest graph's edge count (host int);
        node_off_h / edge_off_h / n_frontier_h = host copies (numpy).  Raises on a non-zero status word (check_status).
        plan=True: the line plan to EVERY frontier slot rides along (drlgx_line_plan over all n_envs x Fmax slots, the unused ones
        planned towards the origin and ignored): actions_pad [n_envs, Fmax, max_actions, 3] f64, n_act_pad [n_envs, Fmax] i32 and
        its host copy n_act_pad_h - the plans' lengths reach the host in the export's own synchronisation."""
        self.use_torch_stream()
        if not hasattr(self, "_gcap"):
            a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
            self._chk(self.L.drlgx_graph_capacity(self.h, C.byref(a), C.byref(b), C.byref(c)))
            self._gcap = (a.value, b.value, c.value)
        mn, me, mf = self._gcap
        dev = self.device
        node_off = torch.empty(self.n_envs + 1, dtype=torch.int32, device=dev)
        edge_off = torch.empty(self.n_envs + 1, dtype=torch.int32, device=dev)
        x = torch.empty(mn, 5, dtype=torch.float32, device=dev)
        ei = torch.empty(2 * me, dtype=torch.int64, device=dev)
        ea = torch.empty(me, dtype=torch.float32, device=dev)
        nfr = torch.empty(self.n_envs, dtype=torch.int32, device=dev)
        fxy = torch.zeros(self.n_envs, mf, 2, dtype=torch.float64, device=dev)
        near = torch.empty(self.n_envs, dtype=torch.int32, device=dev)
        self._chk(self.L.drlgx_graph(self.h, _p(node_off), _p(edge_off), _p(x), _p(ei), _p(ea), _p(nfr), _p(fxy), _p(near)))
        extra = {}
        if plan:
            if getattr(self, "_pad_env", None) is None:
                self._pad_env = torch.arange(self.n_envs, device=dev, dtype=torch.int32).repeat_interleave(mf).contiguous()
            acts, n_act = self.line_plan(self._pad_env, fxy.view(-1, 2))
            extra = dict(actions_pad=acts.view(self.n_envs, mf, -1, 3), n_act_pad=n_act.view(self.n_envs, mf))
        # the batch's boundaries and frontier counts on the host too, with the status word, in ONE synchronisation (keys *_h)
        if plan:
            node_off_h, edge_off_h, nfr_h, n_act_h = self.fetch(node_off, edge_off, nfr, extra["n_act_pad"])
            extra["n_act_pad_h"] = n_act_h
        else:
            node_off_h, edge_off_h, nfr_h = self.fetch(node_off, edge_off, nfr)
        N, E = int(node_off_h[-1]), int(edge_off_h[-1])
        counts = (node_off[1:] - node_off[:-1]).to(torch.int64)
        batch = torch.repeat_interleave(torch.arange(self.n_envs, device=dev), counts, output_size=N)
        return dict(x=x[:N], edge_index=ei[:2 * E].view(2, E), edge_attr=ea[:E], node_off=node_off, edge_off=edge_off,
                    batch=batch, n_frontier=nfr, frontier_xy=fxy, nearest_frontier_node=near,
                    max_graph_edges=int(np.diff(edge_off_h).max()) if self.n_envs else 0,
                    node_off_h=node_off_h, edge_off_h=edge_off_h, n_frontier_h=nfr_h, **extra)

    def snapshot(self, slot=0):
        self.use_torch_stream()
        self._chk(self.L.drlgx_snapshot(self.h, slot))

    def restore(self, slot=0):
        self.use_torch_stream()
        self._chk(self.L.drlgx_restore(self.h, slot))

    def inc_stats(self, reset=False):
        """(SLAM updates served by the incremental rank-k path, full solves) since creation / the last reset;
        (-1, -1) when the incremental path is disabled (DRLGX_INCREMENTAL=0 at creation)."""
        out = (C.c_int64 * 2)()
        self._chk(self.L.drlgx_inc_stats_host(self.h, out, 1 if reset else 0))
        return int(out[0]), int(out[1])

    def panel(self, inst):
        """Development aid: (meta [valid, P, L, M], the covariance panel's live extent [3 P + 2 L, 3 + 2 L] or None when it is not
        valid) of instance `inst` - an env, a look-ahead copy or a snapshot instance (snapshot_instance)."""
        meta = np.zeros(4, dtype=np.int32)
        ipt, dpt = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._chk(self.L.drlgx_debug_panel_host(self.h, inst, meta.ctypes.data_as(ipt), None, 0))
        if meta[0] != 1:
            return meta, None
        body = np.zeros((3 * meta[1] + 2 * meta[2], 3 + 2 * meta[2]))
        self._chk(self.L.drlgx_debug_panel_host(self.h, inst, meta.ctypes.data_as(ipt), body.ctypes.data_as(dpt), body.size))
        return meta, body

    def restore_table(self):
        """Development aid: (info, rows) of the compact restore's table - info = dict(entries, entries_16, in_use, items_per_trip),
        rows [entries][4] = (bytes per instance, unit, bytes per unit, sub-slice bytes) as drlgx_debug_restore_table_host lists them."""
        info = np.zeros(4, dtype=np.int32)
        ipt, lpt = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self._chk(self.L.drlgx_debug_restore_table_host(self.h, info.ctypes.data_as(ipt), None, 0))
        rows = np.zeros((int(info[0]), 4), dtype=np.int64)
        self._chk(self.L.drlgx_debug_restore_table_host(self.h, info.ctypes.data_as(ipt), rows.ctypes.data_as(lpt), rows.shape[0]))
        return dict(entries=int(info[0]), entries_16=int(info[1]), in_use=bool(info[2]), items_per_trip=int(info[3])), rows

    def snapshot_instance(self, slot, env):
        """Instance index of env `env` in snapshot slot `slot` (the getters take any instance)."""
        return 2 * self.n_envs + self.n_rollouts + slot * self.n_envs + env

    def timing_enable(self, on=True):
        """on: False / True (spans around what is launched, fused step = 'step') / 2 (per-stage kernels)."""
        self._chk(self.L.drlgx_timing_enable(self.h, int(on)))

    def timing_read(self):
        ms = (C.c_double * _lib.N_TIMERS)()
        n = (C.c_int64 * _lib.N_TIMERS)()
        self._chk(self.L.drlgx_timing_read_host(self.h, ms, n))
        names = ["sim", "slam", "map", "copy", "graph", "step", "t6", "t7"]  # (t6: og_plan's leaf scoring, t7: an empty span)
        return {names[i]: (ms[i], n[i]) for i in range(_lib.N_TIMERS)}

    # ---- getters (host)
    def counts(self, inst):
        out = (C.c_int32 * 5)()
        self._chk(self.L.drlgx_get_counts_host(self.h, inst, out))
        return dict(poses=out[0], landmarks=out[1], factors=out[2], step=out[3], isam_count=out[4])

    def counts_dev(self):
        """[n_envs, 5] int32 CUDA tensor: poses, landmarks, factors, step, isam update count (no sync)."""
        self.use_torch_stream()
        out = torch.empty(self.n_envs, 5, dtype=torch.int32, device=self.device)
        self._chk(self.L.drlgx_counts(self.h, _p(out)))
        return out

    def poses(self, inst):
        P = self.counts(inst)["poses"]
        xyt = np.zeros((P, 3))
        info = np.zeros((P, 3, 3))
        dp = C.POINTER(C.c_double)
        self._chk(self.L.drlgx_get_poses_host(self.h, inst, xyt.ctypes.data_as(dp), info.ctypes.data_as(dp)))
        return xyt, info

    def landmarks(self, inst):
        n = self.counts(inst)["landmarks"]
        keys = np.zeros(n, dtype=np.int32)
        xy = np.zeros((n, 2))
        info = np.zeros((n, 2, 2))
        dp = C.POINTER(C.c_double)
        self._chk(self.L.drlgx_get_landmarks_host(self.h, inst, keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  xy.ctypes.data_as(dp), info.ctypes.data_as(dp)))
        return keys, xy, info

    def cov_traces(self, inst):
        c = self.counts(inst)
        lm = np.zeros(c["landmarks"])
        ps = np.zeros(c["poses"])
        dp = C.POINTER(C.c_double)
        self._chk(self.L.drlgx_get_cov_traces_host(self.h, inst, lm.ctypes.data_as(dp), ps.ctypes.data_as(dp)))
        return lm, ps

    def virtual_map(self, inst):
        V = self.rows * self.cols
        prob = np.zeros(V)
        info = np.zeros((V, 2, 2))
        tr = np.zeros(V)
        upd = np.zeros(V, dtype=np.uint8)
        dp = C.POINTER(C.c_double)
        self._chk(self.L.drlgx_get_virtual_map_host(self.h, inst, prob.ctypes.data_as(dp), info.ctypes.data_as(dp),
                                                    tr.ctypes.data_as(dp), upd.ctypes.data_as(C.POINTER(C.c_uint8))))
        return prob.reshape(self.rows, self.cols), info, tr.reshape(self.rows, self.cols), upd

    def ground_truth(self, inst):
        veh = np.zeros(3)
        lms = np.zeros((max(self.cfg.num_landmarks, 1), 2))
        dp = C.POINTER(C.c_double)
        self._chk(self.L.drlgx_get_ground_truth_host(self.h, inst, veh.ctypes.data_as(dp), lms.ctypes.data_as(dp)))
        return veh, lms[:self.cfg.num_landmarks]

    def adjacency(self, inst):
        c = self.counts(inst)
        N = c["poses"] + c["landmarks"]
        A = np.zeros((N, N))
        X = np.zeros(N)
        dp = C.POINTER(C.c_double)
        self._chk(self.L.drlgx_get_adjacency_host(self.h, inst, A.ctypes.data_as(dp), X.ctypes.data_as(dp)))
        return A, X

    def factors(self, inst):
        m = self.counts(inst)["factors"]
        pose = np.zeros(m, dtype=np.int32)
        key = np.zeros(m, dtype=np.int32)
        b = np.zeros(m)
        r = np.zeros(m)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self._chk(self.L.drlgx_get_factors_host(self.h, inst, pose.ctypes.data_as(ip), key.ctypes.data_as(ip),
                                                b.ctypes.data_as(dp), r.ctypes.data_as(dp)))
        return pose, key, b, r

    def landmark_order(self):
        o = np.zeros(max(self.cfg.num_landmarks, 1), dtype=np.int32)
        self._chk(self.L.drlgx_get_landmark_order_host(self.h, o.ctypes.data_as(C.POINTER(C.c_int32))))
        return o[:self.cfg.num_landmarks]
