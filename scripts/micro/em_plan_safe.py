"""What the tree sampler's obstacle logic costs: the growth loop of k_em_tree over 256 environments, measured as
scripts/micro/em_plan_split.py measures "tree growth" - Engine.rrt_plan to a goal no node can reach with max_tree_nodes = the mean
tree size of an em_plan call at safe_distance 0, so that every tree fills its table: the same loop, the same number of accepted
nodes, no leaves to score; HIP events around the call (they enclose its one synchronisation), median of --repeats after a warm-up -
on the bench's headline state (256 envs, 40 m map, 100 landmarks, warmed with bench.py's script to 36 poses), in three settings:

  * safe_distance 0, opt-in off   the plain growth loop (kSafe = false) - the number to hold against the parent commit's, which
                                  scripts/micro/em_plan_split.py reports as tree_growth_ms_median
  * safe_distance 0, opt-in on    the same instantiation (the engine launches kSafe = true only for a safe_distance > 0)
  * safe_distance 1.0, opt-in on  kSafe = true: isSafe on every sample and waypoint, the retries, the shrink

and, per setting, the mean number of Halton points drawn per accepted node ((halton_next - start) / (n_nodes - 1) over the trees).

    python scripts/micro/em_plan_safe.py [--repeats 5] [--envs 256] >> profiles/em_plan_safe.txt
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
from drl_graph_exploration_amd.planner2d import halton_start_index  # noqa: E402

MAP, NUM_LM = 40, 100
WARM_SCRIPT = [(1, 1, math.pi / 2)] * 4 + [(2, 0, 0), (2, 0, 0), (0, 0, 0.6)] * 10 + [(2, 0, 0)]  # bench.py: -> 36 poses


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--max-nodes", type=float, default=0.5)
    ap.add_argument("--safe-distance", type=float, default=1.0)
    args = ap.parse_args(argv)
    n = args.envs
    cfg = default_config(MAP, num_landmarks=NUM_LM, max_poses=41, max_actions=64)
    eng = Engine(cfg, n, 0)
    from oracle import oracle as O
    starts = np.array([O.start_pose(lo, MAP / 2 + 20) for lo in range(n)]) + np.array([0.3183, -0.2718, 0.1234])
    eng.reset(np.arange(n), np.arange(n), starts=starts)
    for act in WARM_SCRIPT:
        eng.step(torch.tensor([act] * n, dtype=torch.float64, device=eng.device))
    eng.check_status()
    dev = eng.device
    sel = torch.arange(n, dtype=torch.int32, device=dev)
    h0 = halton_start_index(0)
    start = torch.full((n,), h0, dtype=torch.int32, device=dev)
    eng.set_sampler_parameter(args.max_nodes)
    o = eng.em_plan(sel, start, 2048, int(cfg.algorithm))  # the tree size of the plain call (and a warm-up: workspaces, code objects)
    cap = int(round(float(o["n_nodes"].cpu().numpy().mean())))
    nowhere = torch.full((n, 2), 1.0e6, dtype=torch.float64, device=dev)
    nokey = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rows = []
    for obstacles, sd in ((False, 0.0), (True, 0.0), (True, args.safe_distance)):
        eng.set_sampler_obstacles(obstacles)
        eng.set_sampler_parameter(args.max_nodes, safe_distance=sd)
        r = eng.rrt_plan(sel, nokey, nowhere, start, cap)  # warm-up of this setting
        n_nodes, nxt, res = (t.cpu().numpy() for t in (r["n_nodes"], r["halton_next"], r["result"]))
        grown = n_nodes > 1
        tree = timed(lambda: eng.rrt_plan(sel, nokey, nowhere, start, cap), args.repeats)
        rows.append(dict(obstacles=obstacles, safe_distance=sd, tree_growth_nodes=cap, nodes_mean=float(n_nodes.mean()),
                         trees_full=int((n_nodes == cap).sum()), trees_root_only=int((~grown).sum()),
                         drawn_per_accepted_node=float(((nxt - h0)[grown] / (n_nodes[grown] - 1)).mean()) if grown.any() else None,
                         drawn_total=int((nxt - h0).sum()), tree_growth_ms_median=statistics.median(tree),
                         tree_growth_ms=[round(x, 4) for x in tree]))
    eng.check_status()
    print(json.dumps(dict(envs=n, max_nodes=args.max_nodes, lib=os.environ.get("DRLGX_LIB_DEV", "libdrlgx.so"), repeats=args.repeats,
                          settings=rows)))
    eng.close()


if __name__ == "__main__":
    main()
