"""What one EM-baseline decision for a whole vector of environments costs (Engine.em_plan = drlgx_em_plan: the tree per
environment, its leaves as candidates, their expected costs, the pick), on the bench's headline state (256 envs, 40 m map, 100
landmarks, warmed with bench.py's script to 36 poses) with the planner's shipped max_nodes = 0.5.

  * em_plan:     HIP events around the whole call (they enclose its two host synchronisations), median of --repeats;
  * tree growth: the growth loop alone - Engine.rrt_plan to a goal no node can reach with max_tree_nodes = the mean tree size, so
                 that every tree fills its table: the same loop, the same number of nodes, no leaves to score.  This is the number
                 the one-wave / 256-thread forms of k_em_tree are compared by (DRLGX_LIB_DEV names the variant library).

The split into tree / leaves / em_cost (fm2 kernels, k_em_cost) / pick comes from a kernel trace of a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/micro/em_plan_split.py --repeats 1).

    python scripts/micro/em_plan_split.py [--repeats 3] [--envs 256] > profiles/em_plan_split.txt
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--max-nodes", type=float, default=0.5)
    args = ap.parse_args(argv)
    n = args.envs
    cfg = default_config(MAP, num_landmarks=NUM_LM, max_poses=41, max_actions=64)  # (trees over the 80 m map grow deeper than a line plan)
    eng = Engine(cfg, n, 0)
    from oracle import oracle as O
    starts = np.array([O.start_pose(lo, MAP / 2 + 20) for lo in range(n)]) + np.array([0.3183, -0.2718, 0.1234])
    eng.reset(np.arange(n), np.arange(n), starts=starts)
    for act in WARM_SCRIPT:
        eng.step(torch.tensor([act] * n, dtype=torch.float64, device=eng.device))
    eng.check_status()
    dev = eng.device
    sel = torch.arange(n, dtype=torch.int32, device=dev)
    start = torch.full((n,), halton_start_index(0), dtype=torch.int32, device=dev)
    eng.set_sampler_parameter(args.max_nodes)
    o = eng.em_plan(sel, start, 2048, int(cfg.algorithm))  # warm-up: workspaces, code objects
    n_nodes, n_leaves, n_act = (t.cpu().numpy() for t in (o["n_nodes"], o["n_leaves"], o["n_actions"]))
    em = timed(lambda: eng.em_plan(sel, start, 2048, int(cfg.algorithm)), args.repeats)
    cap = int(round(float(n_nodes.mean())))
    nowhere = torch.full((n, 2), 1.0e6, dtype=torch.float64, device=dev)
    nokey = torch.full((n,), -1, dtype=torch.int32, device=dev)
    r = eng.rrt_plan(sel, nokey, nowhere, start, cap)
    assert int(r["n_nodes"].min()) == cap and int(r["result"].max()) == 0
    tree = timed(lambda: eng.rrt_plan(sel, nokey, nowhere, start, cap), max(args.repeats, 5))
    eng.check_status()
    print(json.dumps(dict(envs=n, max_nodes=args.max_nodes, lib=os.environ.get("DRLGX_LIB_DEV", "libdrlgx.so"),
                          nodes_mean=float(n_nodes.mean()), nodes_max=int(n_nodes.max()), leaves_total=int(n_leaves.sum()),
                          leaves_mean=float(n_leaves.mean()), best_plan_actions_mean=float(n_act.mean()), repeats=args.repeats,
                          em_plan_ms_median=statistics.median(em), em_plan_ms=[round(x, 3) for x in em],
                          tree_growth_nodes=cap, tree_growth_ms_median=statistics.median(tree), tree_growth_ms=[round(x, 4) for x in tree])))
    eng.close()


if __name__ == "__main__":
    main()
