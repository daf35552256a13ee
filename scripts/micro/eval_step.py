"""The execution phase of one vector decision of the evaluation driver at 50 envs (map 40, seeds 0..49, every env's plan to its
nearest frontier), timed both ways in one session with HIP events around the phase (warm, median of several repeats, the two
ways alternating; every repeat starts from the same snapshot, restored and drained before the first event):

  * traced:     one Engine.step_plans_traced call and one Engine.fetch of (trace, executed counts, done flags),
  * per action: one Engine.step_plan(map_last_only=False) and one `metrics().cpu()` per action index - how the hand-assembled
                evaluation loops of tests/test_gpu_vecenv.py read their rows.

Also prints the host synchronisations each way issues per decision (counted where the script makes a synchronising call) and
checks that both ways leave the same rows.

    python scripts/micro/eval_step.py [--repeats 9] [--envs 50] > profiles/eval_driver.txt
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from drl_graph_exploration_amd.vecenv import VecExplorationEnv  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--envs", type=int, default=50)
    args = ap.parse_args(argv)
    n = args.envs
    env = VecExplorationEnv(40, n, env_index=0, test=True, n_rollouts=0)
    eng = env.engine
    g = eng.graph(plan=True)
    acts = g["actions_pad"][:, 0].contiguous()
    nact = g["n_act_pad"][:, 0].contiguous()
    kmax = int(g["n_act_pad_h"][:, 0].max())
    eng.snapshot(0)
    syncs = {"traced": 0, "per_action": 0}

    def traced():
        trace, n_exec, done = eng.step_plans_traced(acts, nact, kmax, done_explored=0.85)
        trace_h, n_exec_h, _ = eng.fetch(trace, n_exec, done)
        syncs["traced"] += 1
        return [trace_h[i, :n_exec_h[i], :3] for i in range(n)]

    def per_action():
        rows = [[] for _ in range(n)]
        nact_h = g["n_act_pad_h"][:, 0]
        for k in range(kmax):
            eng.step_plan(acts, nact, k, map_last_only=False)
            m = eng.metrics().cpu().numpy()
            syncs["per_action"] += 1
            for i in range(n):
                if k < nact_h[i]:
                    rows[i].append(m[i])
        return [np.array(r) for r in rows]

    def timed(fn):
        eng.restore(0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    for fn in (traced, per_action):  # warm: code objects, the fetch buffers
        timed(fn)
    syncs = {"traced": 0, "per_action": 0}
    times = {"traced": [], "per_action": []}
    same = True
    for _ in range(args.repeats):
        ta, ra = timed(traced)
        tb, rb = timed(per_action)
        times["traced"].append(ta)
        times["per_action"].append(tb)
        same = same and all(a.tobytes() == b.tobytes() for a, b in zip(ra, rb))
    eng.check_status()
    env.close()
    out = dict(envs=n, actions_per_decision=kmax, repeats=args.repeats, rows_bit_equal=bool(same),
               traced_ms_median=statistics.median(times["traced"]), per_action_ms_median=statistics.median(times["per_action"]),
               traced_ms=[round(t, 4) for t in times["traced"]], per_action_ms=[round(t, 4) for t in times["per_action"]],
               traced_syncs_per_decision=syncs["traced"] / args.repeats, per_action_syncs_per_decision=syncs["per_action"] / args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
