"""What the SLAM-OG-Shannon cost of the candidate plans of one vector decision costs beside the two costs it is built from, on the
bench's headline state (256 envs, 40 m map, 100 landmarks, warmed with bench.py's script to 36 poses) and the line plans to every
frontier (what actions_all_goals makes):

  * slam_og_cost: Engine.slam_og_cost - drlgx_slam_og_cost: argument check, root weights, one launch of k_og_cost for all candidates,
                  the fm2 covariance update with its landmark blocks and the blend, a chunk of 128 candidates at a time,
  * em_cost:      Engine.em_cost - drlgx_em_cost: the same fm2 update (pose blocks only) in front of k_em_cost,
  * og_cost:      Engine.og_cost - drlgx_og_cost: argument check and the one launch of k_og_cost.

Timed in one session and one process with HIP events around each call (the event pair encloses the call's one host
synchronisation), after warm-up, the ways alternating, median of --repeats.

    python scripts/micro/slam_og_cost_vs_em_cost.py [--repeats 9] [--envs 256] > profiles/slam_og_cost_vs_em_cost.txt
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from drl_graph_exploration_amd import default_config  # noqa: E402
from drl_graph_exploration_amd.engine import Engine  # noqa: E402

MAP, NUM_LM = 40, 100
WARM_SCRIPT = [(1, 1, math.pi / 2)] * 4 + [(2, 0, 0), (2, 0, 0), (0, 0, 0.6)] * 10 + [(2, 0, 0)]  # bench.py: -> 36 poses


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--envs", type=int, default=256)
    args = ap.parse_args(argv)
    n = args.envs
    probe = default_config(MAP, num_landmarks=NUM_LM)
    max_poses = len(WARM_SCRIPT) + 1 + probe.max_actions  # the rollouts of the look-ahead add one pose per action
    cfg = default_config(MAP, num_landmarks=NUM_LM, max_poses=max_poses, max_landmarks=100, max_factors=12 * max_poses + 20)
    eng = Engine(cfg, n, 4096)
    ids = np.arange(n)
    eng.reset(ids, ids, los=ids)
    for act in WARM_SCRIPT:
        eng.step(torch.tensor([act] * n, dtype=torch.float64, device=eng.device))
    eng.check_status()
    g = eng.graph(plan=True)
    nfr = g["n_frontier_h"].astype(np.int64)
    mf = g["actions_pad"].shape[1]
    slot = torch.as_tensor(np.concatenate([e * mf + np.arange(k) for e, k in enumerate(nfr)]), device=eng.device)
    cand_env = torch.as_tensor(np.repeat(ids, nfr), dtype=torch.int32, device=eng.device)
    acts = g["actions_pad"].view(n * mf, -1, 3)[slot].contiguous()
    nact = g["n_act_pad"].view(-1)[slot].contiguous()
    kmax = int(nact.max().item())
    alg = int(cfg.algorithm)
    alpha = 0.5  # EMPlannerParameter's default

    ways = {"slam_og_cost": lambda: eng.slam_og_cost(cand_env, acts, nact, alpha), "em_cost": lambda: eng.em_cost(cand_env, acts, nact, alg),
            "og_cost": lambda: eng.og_cost(cand_env, acts, nact)}

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    for fn in ways.values():  # warm: code objects, the lazily allocated workspaces
        timed(fn)
        timed(fn)
    times = {k: [] for k in ways}
    outs = {}
    for _ in range(args.repeats):
        for k, fn in ways.items():
            t, outs[k] = timed(fn)
            times[k].append(t)
    eng.check_status()
    unc, cost = (t.cpu().numpy() for t in outs["slam_og_cost"])
    raw_og = -outs["og_cost"][1].cpu().numpy()
    first = np.cumsum(nfr) - nfr
    agree = [int(np.argmin(cost[f:f + k]) == np.argmax(raw_og[f:f + k])) for f, k in zip(first, nfr) if k > 1]
    counts = eng.fetch(eng.counts_dev())[0]
    out = dict(envs=n, candidates=int(cand_env.numel()), mean_actions=float(nact.float().mean().item()), max_actions_in_plans=kmax,
               poses=int(counts[:, 0].max()), landmarks_mean=float(counts[:, 1].mean()), cells=eng.rows * eng.cols, repeats=args.repeats,
               finite_costs=bool(np.isfinite(cost).all()), same_best_frontier_as_og_fraction=(sum(agree) / len(agree)) if agree else None)
    for k in ways:
        out[k + "_ms_median"] = statistics.median(times[k])
        out[k + "_ms"] = [round(t, 4) for t in times[k]]
    out["slam_og_cost_over_em_cost"] = out["slam_og_cost_ms_median"] / out["em_cost_ms_median"]
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
