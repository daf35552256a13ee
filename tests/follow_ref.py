"""TEST INFRASTRUCTURE: drlgx_follow_plans restated in plain Python on top of one Engine.step per action - the selection rule of
explore()'s switch on the planner's result and the stops of EMExplorer.follow_path (scripts/envs/pyplanner2d.py:100-109,170-187)
plus the evaluation loop's `done` (scripts/test.py:128-152) - and the eight-environment world tests/test_gpu_follow.py runs it on.

World: environment e around its own centre (13 m apart), heading along +x, a landmark K 0.6 m ahead of the centre and a far one; it
starts at the centre ('near': K is 0.4 m inside safe_distance = 1.0, so the first step that moves is flagged) or 1.4 m behind it
('far': K at 2.0 m; FWD twice brings it to 1.3 m, then 0.6 m).  A quiet vehicle (translation noise 0.01 m) keeps every distance
0.25 m and more from safe_distance."""
import math

import numpy as np
import torch

SUCCESS, SAMPLING_FAILURE, NO_SOLUTION, TERMINATION = 3, 0, 1, 2
RAN, DONE, OBSTACLE, REJECTED, STOP_NO_SOLUTION, STOP_TERMINATION = range(6)
FALLBACK = (0.0, 0.0, math.pi / 4)
SAFE = 1.0
MAP = 40
N = 8
A_MAX = 6
CENTRES = [(-19.5 + 13.0 * (e % 4) + 0.3183, (-10.0 if e < 4 else 10.0) - 0.2718) for e in range(N)]
HEADING = 0.0234
FWD, JIG, JAG, STAY, REJECT = (0.7, 0.0, 0.0), (0.05, 0.0, 0.01), (-0.05, 0.0, -0.01), (0.0, 0.0, 0.0), (100.0, 0.0, 0.0)


def _rel(e, x, y):
    c, s = math.cos(HEADING), math.sin(HEADING)
    return (CENTRES[e][0] + c * x - s * y, CENTRES[e][1] + s * x + c * y)


def fixed_landmarks():
    return np.array([p for e in range(N) for p in (_rel(e, 0.6, 0.0), _rel(e, 3.0, 1.5))])


def starts(where):
    return np.array([_rel(e, -1.4 if where[e] == "far" else 0.0, 0.0) + (HEADING,) for e in range(N)])


def engine_config(safe_distance=SAFE):
    from drl_graph_exploration_amd import default_config
    cfg = default_config(MAP, num_landmarks=2 * N, max_poses=12, max_landmarks=8, max_factors=256, max_actions=A_MAX)
    cfg.safe_distance = safe_distance
    cfg.translation_noise = 0.01
    return cfg


def in_box(cfg, a):
    """SS2D.simulate's test of an odometry increment (pyss2d.py:173-176)."""
    return cfg.map_min_x < a[0] < cfg.map_max_x and cfg.map_min_y < a[1] < cfg.map_max_y


def select(plans, results, active, steps):
    """Per env (its actions, its stop code before anything runs)."""
    out = []
    for e in range(len(plans)):
        on = active is None or bool(active[e])
        if on and results[e] == SUCCESS:
            out.append((list(plans[e][:max(steps, 0)]), RAN))
        elif on and results[e] == SAMPLING_FAILURE:
            out.append(([FALLBACK], RAN))
        else:
            out.append(([], {NO_SOLUTION: STOP_NO_SOLUTION, TERMINATION: STOP_TERMINATION}.get(results[e], RAN)))
    return out


def follow_stepwise(eng, plans, results, active, steps, sigma0=1.0, done_explored=0.85, max_steps=5000):
    """The same actions one Engine.step at a time, the flags, metrics and counters read after each.  Returns (rows [env] -> list of
    4-tuples, n_exec, done, stop)."""
    n = eng.n_envs
    sel = select(plans, results, active, steps)
    acts = [s[0] for s in sel]
    stop = [s[1] for s in sel]
    live = [len(a) > 0 for a in acts]
    rows = [[] for _ in range(n)]
    done = [0] * n
    for a in range(max([len(x) for x in acts] + [0])):
        odom = np.zeros((n, 3))
        mask = np.zeros(n, dtype=np.uint8)
        for e in range(n):
            if live[e] and a >= len(acts[e]):
                live[e] = False
            if live[e] and not in_box(eng.cfg, acts[e][a]):  # a rejected odometry executes nothing and stops the env there
                live[e], stop[e] = False, REJECTED
            if live[e]:
                odom[e], mask[e] = acts[e][a], 1
        if not mask.any():
            break
        eng.step(torch.tensor(odom, dtype=torch.float64, device=eng.device), torch.tensor(mask, device=eng.device))
        flag, m, ex = eng.fetch(eng.obstacle_flags()[0], eng.metrics(sigma0), eng.explored())
        for e in range(n):
            if not mask[e]:
                continue
            rows[e].append((m[e, 0], m[e, 1], m[e, 2], ex[e]))
            if ex[e] > done_explored or eng.counts(e)["step"] > max_steps:
                done[e], stop[e], live[e] = 1, DONE, False
            elif flag[e]:
                stop[e], live[e] = OBSTACLE, False
    return rows, [len(r) for r in rows], done, stop


def tensors(eng, plans, results, active):
    plan = torch.zeros(eng.n_envs, A_MAX, 3, dtype=torch.float64, device=eng.device)
    for e, p in enumerate(plans):
        if len(p):
            plan[e, :len(p)] = torch.tensor(p, dtype=torch.float64)
    n_act = torch.tensor([len(p) for p in plans], dtype=torch.int32, device=eng.device)
    res = torch.tensor(results, dtype=torch.int32, device=eng.device)
    act = None if active is None else torch.tensor(active, dtype=torch.uint8, device=eng.device)
    return plan, n_act, res, act
