"""The EM-exploration baseline's episodes in the evaluation CSV format (the counterpart of evaluate.py for the planner of
scripts/envs/pyplanner2d.py:155-195): all seeds in one VecExplorationEnv(test=True); per vector decision one em_plan with the
planner's safe_distance, one follow (Engine.follow_plans, with SS2D.simulate's obstacle flag at the environment's safe_distance)
and one fetch.  An episode ends on done, NO_SOLUTION, TERMINATION or a travelled distance above max_distance.

    python -m drl_graph_exploration_amd.em_baseline [--algorithm EM_AOPT|EM_DOPT|OG_SHANNON|SLAM_OG_SHANNON] [--alpha 0.5]
                                                    [--map-size 40] [--seeds 50] [--first-seed 0] [--steps 5] [--max-distance 450]
                                                    [--max-decisions N] [--out DIR]

Served: the non-Dubins control model under all four OptimizationAlgorithms - the EM algorithms as the reference's
exploration_env.ini ships them, and the two occupancy-grid baselines (Engine.og_plan; --alpha is SLAM_OG_SHANNON's weight of the
landmark term)."""
import argparse
import os
import time

import numpy as np
import torch

from . import evaluate as ev

ALGORITHMS = {"EM_AOPT": 0, "EM_DOPT": 1, "OG_SHANNON": 2, "SLAM_OG_SHANNON": 3}
PLANNER_SAFE_DISTANCE = 1.0   # exploration_env.ini [Planner] safe_distance ([Environment] safe_distance is 0 there, and in default_config)
MAX_NODES = 0.5


def csv_path(out_dir, map_size, algorithm):
    return os.path.join(out_dir, "%d_EM_%s.csv" % (map_size, algorithm))


def run(algorithm="EM_AOPT", map_size=40, seeds=50, steps=5, max_distance=450.0, max_decisions=None, device=0, sigma0=1.0,
        max_poses=256, planner_safe_distance=PLANNER_SAFE_DISTANCE, max_tree_nodes=2048, alpha=None):
    """Records of the shape evaluate.evaluate returns - dict(seed, done, stalled, decisions=[dict(time, plan, rows, explored,
    result, stop)]) plus `status` (DONE, NO SOLUTION, TERMINATION, MAX_DISTANCE or None while the episode still runs) - `time` being
    the batched planning wall time divided by the live envs.  `alpha` (None: EMPlannerParameter's default): the planner parameter
    that SLAM_OG_SHANNON reads."""
    from .vecenv import VecExplorationEnv
    seeds = list(range(int(seeds))) if np.isscalar(seeds) else [int(s) for s in seeds]
    n = len(seeds)
    if n == 0:
        return []
    env = VecExplorationEnv(map_size, n, env_index=seeds, test=True, max_poses=max_poses, n_rollouts=0, device=device,
                            algorithm=ALGORITHMS[algorithm], alpha=alpha)
    dev = env.device
    records = [dict(seed=int(s), done=False, stalled=False, status=None, decisions=[]) for s in env.env_index]
    live = np.ones(n, dtype=bool)
    d = 0
    try:
        env.engine.set_env_obstacles(True)  # (live once the config's [Environment] safe_distance is positive; inert at the shipped 0)
        while live.any() and (max_decisions is None or d < max_decisions):
            active = torch.as_tensor(live.astype(np.uint8), device=dev)
            torch.cuda.synchronize(dev)
            t0 = time.time()
            plan, n_act, result = env.em_plan(MAX_NODES, max_tree_nodes, safe_distance=planner_safe_distance)
            torch.cuda.synchronize(dev)
            plan_time = (time.time() - t0) / int(live.sum())
            trace, n_exec, done, stop = env.follow(plan, n_act, result, steps=steps, active=active, sigma0=sigma0)
            trace_h, nexec_h, done_h, stop_h, plan_h, nact_h, res_h, dist_h = env.engine.fetch(trace, n_exec, done, stop, plan, n_act, result,
                                                                                               env.dist)
            for i in np.nonzero(live)[0]:
                rec, k = records[i], int(nexec_h[i])
                rec["decisions"].append(dict(time=plan_time, plan=plan_h[i, :nact_h[i]].tolist(), rows=trace_h[i, :k, :3].tolist(),
                                             explored=trace_h[i, :k, 3].tolist(), result=int(res_h[i]), stop=int(stop_h[i])))
                if done_h[i]:
                    rec["done"], rec["status"] = True, "DONE"
                elif stop_h[i] == env.engine.STOP_NO_SOLUTION:
                    rec["status"] = "NO SOLUTION"
                elif stop_h[i] == env.engine.STOP_TERMINATION:
                    rec["status"] = "TERMINATION"
                elif dist_h[i] > max_distance:
                    rec["status"] = "MAX_DISTANCE"
                live[i] = rec["status"] is None
            d += 1
    finally:
        env.close()
    return records


def build_parser():
    from .planner2d import EMPlannerParameter
    ap = argparse.ArgumentParser(description="EM-exploration baseline episodes in the evaluation CSV format")
    ap.add_argument("--algorithm", default="EM_AOPT", choices=sorted(ALGORITHMS))
    ap.add_argument("--alpha", type=float, default=EMPlannerParameter().alpha, help="SLAM_OG_SHANNON's weight of the landmark term")
    ap.add_argument("--map-size", type=int, default=40, choices=sorted(ev.PLOT_MAX_STEP))
    ap.add_argument("--seeds", type=int, default=50)
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--max-distance", type=float, default=450.0)
    ap.add_argument("--max-decisions", type=int, default=None)
    ap.add_argument("--out", default=".")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    seeds = list(range(args.first_seed, args.first_seed + args.seeds))
    records = run(args.algorithm, args.map_size, seeds, steps=args.steps, max_distance=args.max_distance, max_decisions=args.max_decisions,
                  alpha=args.alpha)
    os.makedirs(args.out, exist_ok=True)
    path = csv_path(args.out, args.map_size, args.algorithm)
    ev.write_csv(records, path, "EM+" + args.algorithm, args.map_size)
    print("%s: %d seeds, %s" % (path, len(records), ", ".join("%s %s" % (r["seed"], r["status"]) for r in records)))
    return path


if __name__ == "__main__":
    main()
