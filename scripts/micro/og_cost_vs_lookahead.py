"""What scoring the candidate plans of one vector decision costs the three ways, on the bench's headline state (256 envs, 40 m map,
100 landmarks, warmed with bench.py's script to 36 poses) and the line plans to every frontier (what actions_all_goals makes):

  * og_cost:    Engine.og_cost - the expected map entropy (drlgx_og_cost: argument check, one launch of k_og_cost for all candidates),
  * em_cost:    Engine.em_cost - the deterministic expected EM cost (drlgx_em_cost: the fm2 covariance update in front of k_em_cost),
  * lookahead:  Engine.lookahead (drlgx_lookahead_bounded) - the stochastic look-ahead on the same candidates.

Timed in one session with HIP events around each call (the event pair encloses the one host synchronisation of og_cost / em_cost),
after warm-up, the ways alternating, median of --repeats.

    python scripts/micro/og_cost_vs_lookahead.py [--repeats 9] [--envs 256] > profiles/og_cost_vs_lookahead.txt
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

    ways = {"og_cost": lambda: eng.og_cost(cand_env, acts, nact), "em_cost": lambda: eng.em_cost(cand_env, acts, nact, alg),
            "lookahead": lambda: eng.lookahead(cand_env, acts, nact, max_n_actions=kmax)}

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
    ent, cost = (t.cpu().numpy() for t in outs["og_cost"])
    zeros = torch.zeros(n, dtype=torch.int32, device=eng.device)
    root = eng.og_cost(torch.arange(n, dtype=torch.int32, device=eng.device), acts.new_zeros((n,) + tuple(acts.shape[1:])), zeros)[0]
    raw_og = root[cand_env.long()].cpu().numpy() - cost
    raw_sim = outs["lookahead"].cpu().numpy()
    first = np.cumsum(nfr) - nfr
    agree = [int(np.argmax(raw_og[f:f + k]) == np.argmax(raw_sim[f:f + k])) for f, k in zip(first, nfr) if k > 1]
    counts = eng.fetch(eng.counts_dev())[0]
    out = dict(envs=n, candidates=int(cand_env.numel()), mean_actions=float(nact.float().mean().item()), max_actions_in_plans=kmax,
               poses=int(counts[:, 0].max()), landmarks_mean=float(counts[:, 1].mean()), cells=eng.rows * eng.cols, repeats=args.repeats,
               same_best_frontier_fraction=(sum(agree) / len(agree)) if agree else None)
    for k in ways:
        out[k + "_ms_median"] = statistics.median(times[k])
        out[k + "_ms"] = [round(t, 4) for t in times[k]]
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
