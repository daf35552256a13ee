"""What the tree sampler's Dubins control model costs, and that the plain and obstacle loops cost what they did: the growth loop of
k_em_tree over 256 environments, measured as scripts/micro/em_plan_safe.py measures it - Engine.rrt_plan to a goal no node can reach,
max_tree_nodes = the mean tree size of an em_plan call at safe_distance 0, HIP events around the call (they enclose its one
synchronisation), median of --repeats after a warm-up - on the bench's headline state (256 envs, 40 m map, 100 landmarks, warmed
with bench.py's script to 36 poses):

  (a) the plain loop (safe_distance 0) and the obstacle loop (safe_distance 1.0 behind the opt-in) - to hold against the parent
      commit's library in the same session (DRLGX_LIB_DEV names the library; --no-dubins for a library without the feature);
  (b) the Dubins loop with the 320-entry library of tests/em_dubins_cases.py and with the [Dubins] section the reference ships
      (78 030 entries), with and without the exact pre-filter: the Halton points drawn per accepted node and the library entries a
      scan without the pre-filter looks at per accepted node (refused connects scan the whole library; an accepted one up to the end
      of the winner's stride of 64).  A tree whose connect counter fires (1001 refused in a row) ends early: trees_failed.

    python scripts/micro/em_plan_dubins.py [--repeats 5] [--envs 256] [--no-dubins] >> profiles/em_plan_dubins.txt

--optimize2: what one EM-baseline decision costs under the Dubins control model instead (Engine.em_plan behind
set_dubins_leaf_scoring: the Dubins tree with optimize2's stop rule, every leaf scored with its non-core steps, the pick), per
library: HIP events around the whole call, and around Engine.em_cost(core, distance) on the leaves read back - the share of the
scoring (argument check, prior, covariance update, k_em_cost); the rest is tree + leaves + pick.  The engine of this mode has
max_actions = 128 (a plan has one row per STEP, up to 20 per edge with the shipped library), and max_nodes starts at
--optimize2-max-nodes and is halved while a leaf deeper than that refuses the call.  The per-kernel split (k_em_tree /
k_em_leaves_dubins / k_fm2_check, k_fm2_prior, k_fm2_update, k_em_cost / k_em_pick) comes from a kernel trace of a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/micro/em_plan_dubins.py --optimize2 --repeats 1).

    python scripts/micro/em_plan_dubins.py --optimize2 [--repeats 5] [--envs 256] >> profiles/em_plan_dubins_optimize2.txt
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
#            max_w dw    min_v max_v dv    dt   min_d max_d tolerance
LIBRARIES = {"320": (0.7, 0.1, 0.6, 1.0, 0.1, 0.5, 1.0, 3.0, 0.6), "shipped": (0.5, 0.01, 0.5, 1.0, 0.01, 0.2, 1.0, 4.0, 0.3)}


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


def optimize2(args):
    from drl_graph_exploration_amd._lib import DrlgxError
    n = args.envs
    cfg = default_config(MAP, num_landmarks=NUM_LM, max_poses=41, max_actions=128)
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
    eng.set_dubins_leaf_scoring(True)
    rows = []
    for name, params in LIBRARIES.items():
        size = eng.set_dubins_library(params)
        max_nodes, refused, o = args.optimize2_max_nodes, 0, None
        while o is None:
            eng.set_sampler_parameter(max_nodes, dubins_control_model_enabled=True)
            try:
                o = eng.em_plan(sel, start, 2048, int(cfg.algorithm))  # (and the warm-up of this setting)
            except DrlgxError:
                refused, max_nodes = refused + 1, max_nodes / 2
        n_nodes, n_leaves, n_act, res, nxt = (o[k].cpu().numpy() for k in ("n_nodes", "n_leaves", "n_actions", "result", "halton_next"))
        lv = eng.em_plan_leaves()
        whole = timed(lambda: eng.em_plan(sel, start, 2048, int(cfg.algorithm)), args.repeats)
        score = timed(lambda: eng.em_cost(lv["cand_env"], lv["actions"], lv["n_actions"], int(cfg.algorithm), core=lv["core"],
                                          distance=lv["distance"]), args.repeats)
        steps = lv["n_actions"].cpu().numpy()
        rows.append(dict(setting="optimize2, dubins %s" % name, library=size, max_nodes=max_nodes, calls_refused_for_depth=refused,
                         nodes_mean=float(n_nodes.mean()), trees_failed=int((res == 0).sum()), leaves_total=int(n_leaves.sum()),
                         leaf_steps_mean=float(steps.mean()) if len(steps) else 0.0, leaf_steps_max=int(steps.max()) if len(steps) else 0,
                         core_steps_mean=float(lv["core"].sum(dim=1).double().mean()) if len(steps) else 0.0,
                         best_plan_steps_mean=float(n_act.mean()), drawn_total=int((nxt - h0).sum()),
                         em_plan_ms_median=statistics.median(whole), em_plan_ms=[round(x, 3) for x in whole],
                         em_cost_on_leaves_ms_median=statistics.median(score), em_cost_on_leaves_ms=[round(x, 3) for x in score],
                         tree_leaves_pick_ms=statistics.median(whole) - statistics.median(score)))
    eng.check_status()
    print(json.dumps(dict(envs=n, lib=os.environ.get("DRLGX_LIB_DEV", "libdrlgx.so"), repeats=args.repeats, settings=rows)))
    eng.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--max-nodes", type=float, default=0.5)
    ap.add_argument("--safe-distance", type=float, default=1.0)
    ap.add_argument("--no-dubins", action="store_true")
    ap.add_argument("--optimize2", action="store_true")
    ap.add_argument("--optimize2-max-nodes", type=float, default=0.1)
    args = ap.parse_args(argv)
    if args.optimize2:
        return optimize2(args)
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

    def measure(tag, want_nodes=False, **extra):
        r = eng.rrt_plan(sel, nokey, nowhere, start, cap, want_nodes=want_nodes)  # warm-up of this setting
        n_nodes, nxt, res = (t.cpu().numpy() for t in (r["n_nodes"], r["halton_next"], r["result"]))
        grown = n_nodes > 1
        tree = timed(lambda: eng.rrt_plan(sel, nokey, nowhere, start, cap), args.repeats)
        row = dict(setting=tag, tree_growth_nodes=cap, nodes_mean=float(n_nodes.mean()), trees_full=int((n_nodes == cap).sum()),
                   trees_root_only=int((~grown).sum()),
                   drawn_per_accepted_node=float((nxt - h0).sum() / max(int((n_nodes - 1).sum()), 1)),
                   drawn_total=int((nxt - h0).sum()), tree_growth_ms_median=statistics.median(tree),
                   tree_growth_ms=[round(x, 4) for x in tree], **extra)
        rows.append(row)
        return r, n_nodes, nxt

    for obstacles, sd in ((False, 0.0), (True, args.safe_distance)):
        eng.set_sampler_obstacles(obstacles)
        eng.set_sampler_parameter(args.max_nodes, safe_distance=sd)
        measure("obstacles" if obstacles else "plain", safe_distance=sd)
    eng.set_sampler_obstacles(False)
    if not args.no_dubins:
        for name, params in LIBRARIES.items():
            size = eng.set_dubins_library(params)
            eng.set_sampler_parameter(args.max_nodes, dubins_control_model_enabled=True)
            for prefilter in (True, False):
                eng.set_dubins_prefilter(prefilter)
                r, n_nodes, nxt = measure("dubins %s, pre-filter %s" % (name, "on" if prefilter else "off"), want_nodes=True, library=size)
                nodes = r["nodes"].cpu().numpy()
                accepted = int((n_nodes - 1).sum())
                refused = int((nxt - h0).sum()) - accepted
                idx = np.concatenate([nodes[i, 1:n_nodes[i], 5] for i in range(n)]).astype(np.int64) if accepted else np.zeros(0, np.int64)
                scanned = refused * size + int(np.minimum((idx // 64 + 1) * 64, size).sum())
                rows[-1].update(trees_failed=int((n_nodes < cap).sum()), refused_connects=refused,
                                scanned_entries_per_accepted_node_unfiltered=scanned / max(accepted, 1))
            eng.set_dubins_prefilter(True)
        eng.set_sampler_parameter(args.max_nodes)
    eng.check_status()
    print(json.dumps(dict(envs=n, max_nodes=args.max_nodes, lib=os.environ.get("DRLGX_LIB_DEV", "libdrlgx.so"), repeats=args.repeats,
                          settings=rows)))
    eng.close()


if __name__ == "__main__":
    main()
