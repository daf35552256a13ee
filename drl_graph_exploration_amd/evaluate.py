"""`test.py` of the reference (scripts/test.py) over the drlgx engine: a trained policy drives the seeded test maps greedily and
the per-action metrics are written as `<data_root>/test_result/<map>_<method>_<model>.csv`, in the reference's file format.

    python -m drl_graph_exploration_amd.evaluate <DQN|A2C> <GCN|GG-NN|g-U-Net> [--map-size 40|60|80|100] [--seeds 50]
        [--first-seed 0] [--weights PATH] [--data-root ../data] [--out DIR] [--max-decisions N]

All seeds run in ONE `VecExplorationEnv(test=True)`.  A vector decision (scripts/test.py:96-152 for every live env) is

    graph_matrix(plan=True)     the batched graphs and the line plan to every frontier (its own synchronisation: the batch's sizes)
    forward                     `test_q` with p = 0 (DQN) or `test_a2c` (A2C) over the whole batch
    Engine.greedy_plans         arg-max over every env's frontier scores and the chosen plan, on the device
    step_traced                 the plans action by action: a metric row per executed action, an env stops where it is done

and the host reads the rows, the executed counts, the done flags, the choices and the status word with one `engine.fetch`: one
synchronisation for the execution of a decision instead of one per executed action.  Finished envs ride along inactive.

Differences from the reference, on purpose:

* `Computation time` is the wall time of the BATCHED forward (synchronised before and after) divided by the number of live envs:
  a share of a batch's latency, not the reference's latency of one graph on its own.
* An env that is not done but has no frontier left would spin forever in the reference (`np.argmax` of an empty list raises
  there); here it is marked stalled and ends like a finished one.  The number of stalled envs is printed.
"""
import argparse
import os
import time

import numpy as np
import torch

from . import networks
from .policy import _is_rank0

HEADER = "Category,Computation time,Map size,Landmarks error,Map entropy,Max localization uncertainty,Step"
PLOT_MAX_STEP = {40: 400, 60: 1200, 80: 2400, 100: 4500}  # scripts/test.py:25-32
METHODS = ("DQN", "A2C")
MODEL_NAMES = ("GCN", "GG-NN", "g-U-Net")
_UNET_ARGS = (5, 1000, 1000, 3)  # in_channels, hidden_channels, out_channels, depth (scripts/test.py:42, 54)
_TABLE = {
    ("DQN", "GCN"): ("GCN", ()), ("DQN", "GG-NN"): ("GGNN", ()), ("DQN", "g-U-Net"): ("GraphUNet", _UNET_ARGS),
    ("A2C", "GCN"): ("PolicyGCN", ()), ("A2C", "GG-NN"): ("PolicyGGNN", ()), ("A2C", "g-U-Net"): ("PolicyGraphUNet", _UNET_ARGS),
}


def model_spec(method, model):
    """(class, constructor arguments) of scripts/test.py:35-58 for a (training method, model name) pair."""
    if (method, model) not in _TABLE:
        raise ValueError("method is one of %s and model one of %s, got %r %r" % (METHODS, MODEL_NAMES, method, model))
    name, args = _TABLE[(method, model)]
    return getattr(networks, name), args


def build_model(method, model):
    cls, args = model_spec(method, model)
    return cls(*args)


def default_weights(data_root, method, model):
    return os.path.join(data_root, "torch_weights", method + "_" + model, "MyModel.pt")


def csv_path(out_dir, map_size, method, model):
    return os.path.join(out_dir, "%d_%s_%s.csv" % (map_size, method, model))


def evaluate(method, model, map_size=40, seeds=50, max_decisions=None, weights=None, data_root="../data", net=None, device=0,
             sigma0=1.0, max_poses=256, keep_scores=False):
    """Run the greedy policy on the test maps `seeds` (a count: 0 .. seeds - 1, or a list of seeds).  Returns one record per
    seed: dict(seed, done, stalled, decisions=[dict(time, choice, goal, plan, rows, explored)]), rows = [[landmark error, map
    entropy, max localisation uncertainty], ...] of the executed actions, plan = the chosen line plan ([k, 3]; an episode that
    ends inside it executed len(rows) of them), explored = the explored share after each action.  max_decisions: stop there.
    keep_scores: every decision also carries `scores`, the network's output over the env's frontiers (what the pick saw)."""
    from .networks import GraphData
    from .vecenv import VecExplorationEnv
    seeds = list(range(int(seeds))) if np.isscalar(seeds) else [int(s) for s in seeds]
    n = len(seeds)
    if n == 0:
        return []
    env = VecExplorationEnv(map_size, n, env_index=seeds, test=True, max_poses=max_poses, n_rollouts=0, device=device)
    dev = env.device
    if net is None:
        net = build_model(method, model)
        path = weights if weights is not None else default_weights(data_root, method, model)
        net.load_state_dict(torch.load(path, map_location="cpu"))
    net.to(dev).eval()
    # (the seed an env runs on: reset() moves a map without a landmark in sight to seed + 50, as the reference does)
    records = [dict(seed=int(s), done=False, stalled=False, decisions=[]) for s in env.env_index]
    live = np.ones(n, dtype=bool)
    rows_env = torch.arange(n, device=dev)
    d = 0
    try:
        while live.any() and (max_decisions is None or d < max_decisions):
            g = env.graph_matrix(plan=True)
            nfr = g["n_frontier"]
            data = GraphData(g["x"], g["edge_index"], g["edge_attr"], g["batch"], g["node_off"], g["edge_off"], g["max_graph_edges"])
            torch.cuda.synchronize(dev)
            t0 = time.time()
            with torch.no_grad():
                if method == "DQN":  # test_q(s_t, 0, ...): the per-node read-out, the frontiers are each graph's last nodes
                    score = net(data, 0.0, batch=g["batch"]).view(-1).float()
                    seg_begin = g["node_off"][1:] - nfr
                else:                # test_a2c: the soft-max over the frontier nodes, compact and env-major
                    end = g["node_off"][1:].long()[g["batch"]]
                    mask = torch.arange(g["x"].shape[0], device=dev) >= end - nfr.long()[g["batch"]]
                    data.n_masked = int(g["n_frontier_h"].astype(np.int64).sum())
                    score = net(data, mask, batch=g["batch"]).view(-1).float()
                    seg_begin = (torch.cumsum(nfr, 0) - nfr).to(torch.int32)
            torch.cuda.synchronize(dev)
            policy_time = (time.time() - t0) / int(live.sum())
            active = torch.as_tensor(live.astype(np.uint8), device=dev)
            choice, acts, nact = env.engine.greedy_plans(score, seg_begin, nfr, g["actions_pad"], g["n_act_pad"], active)
            goal = g["frontier_xy"][rows_env, choice.clamp(min=0).long()]
            # a host bound of the chosen plans' lengths: the longest plan to a frontier of a live env (from the export's own read)
            slots = np.arange(g["n_act_pad_h"].shape[1])[None, :] < g["n_frontier_h"][:, None]
            lens = g["n_act_pad_h"][slots & live[:, None]]
            kmax = int(lens.max()) if lens.size else 0
            trace, n_exec, done = env.step_traced(acts, nact, kmax=kmax, sigma0=sigma0)
            more = (score, seg_begin.to(torch.int32)) if keep_scores else ()
            trace_h, nexec_h, done_h, choice_h, nact_h, acts_h, goal_h, *more_h = env.engine.fetch(trace, n_exec, done, choice, nact, acts, goal,
                                                                                                 *more)
            for i in np.nonzero(live)[0]:
                rec = records[i]
                if choice_h[i] < 0:
                    rec["stalled"] = True
                    live[i] = False
                    continue
                k = int(nexec_h[i])
                rec["decisions"].append(dict(time=policy_time, choice=int(choice_h[i]), goal=goal_h[i].tolist(),
                                             plan=acts_h[i, :nact_h[i]].tolist(), rows=trace_h[i, :k, :3].tolist(),
                                             explored=trace_h[i, :k, 3].tolist()))
                if keep_scores:
                    b = int(more_h[1][i])
                    rec["decisions"][-1]["scores"] = more_h[0][b:b + int(g["n_frontier_h"][i])].copy()
                if done_h[i]:
                    rec["done"] = True
                    live[i] = False
            d += 1
    finally:
        env.close()
    return records


def _f(v):
    return repr(float(v))  # the shortest string that reads back as the same double: what pandas' to_csv writes


def csv_lines(records, category, map_size):
    """The reference's data frame as text lines (scripts/test.py:124-152, 204-211): per decision one `Computation time` row, per
    executed action one metric row with the running step; a finished episode repeats its last row up to plot_max_step."""
    plot_max_step = PLOT_MAX_STEP[int(map_size)]
    lines = [HEADER]
    for rec in records:
        step, last = 0, None
        for dec in rec["decisions"]:
            lines.append("%s,%s,%s,,,," % (category, _f(dec["time"]), _f(map_size)))
            for row in dec["rows"]:
                step += 1
                last = "%s,,,%s,%s,%s," % (category, _f(row[0]), _f(row[1]), _f(row[2]))
                lines.append(last + _f(step))
        if (rec.get("done") or rec.get("stalled")) and last is not None:
            while step < plot_max_step:
                step += 1
                lines.append(last + _f(step))
    return lines


def write_csv(records, path, category, map_size):
    """Write the records as the reference's CSV (seeds one after another).  Rank 0 only, through a temporary file + os.replace
    (like policy.save_state_dict): a reader never sees half a file."""
    if not _is_rank0():
        return
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w", newline="") as f:
        f.write("\n".join(csv_lines(records, category, map_size)) + "\n")
    os.replace(tmp, path)


def main(argv=None):
    ap = argparse.ArgumentParser(description="scripts/test.py of the reference over the drlgx engine")
    ap.add_argument("training_method", choices=list(METHODS))
    ap.add_argument("model_name", choices=list(MODEL_NAMES))
    ap.add_argument("--map-size", type=int, default=40, choices=sorted(PLOT_MAX_STEP))
    ap.add_argument("--seeds", type=int, default=50, help="number of test maps (the reference: 50)")
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--weights", default=None, help="default: <data-root>/torch_weights/<method>_<model>/MyModel.pt")
    ap.add_argument("--data-root", default="../data")
    ap.add_argument("--out", default=None, help="default: <data-root>/test_result")
    ap.add_argument("--max-decisions", type=int, default=None, help="stop every episode after N decisions (default: run to done)")
    args = ap.parse_args(argv)
    seeds = list(range(args.first_seed, args.first_seed + args.seeds))
    records = evaluate(args.training_method, args.model_name, args.map_size, seeds, max_decisions=args.max_decisions,
                       weights=args.weights, data_root=args.data_root)
    out_dir = args.out if args.out is not None else os.path.join(args.data_root, "test_result")
    os.makedirs(out_dir, exist_ok=True)
    path = csv_path(out_dir, args.map_size, args.training_method, args.model_name)
    write_csv(records, path, args.training_method + "+" + args.model_name, args.map_size)
    n_done = sum(r["done"] for r in records)
    n_stalled = sum(r["stalled"] for r in records)
    print("%s: %d seeds, %d done, %d stalled (no frontier left), %d steps" %
          (path, len(records), n_done, n_stalled, sum(len(d["rows"]) for r in records for d in r["decisions"])))
    return path


if __name__ == "__main__":
    main()
