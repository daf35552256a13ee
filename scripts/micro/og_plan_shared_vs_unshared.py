"""What the shared base of drlgx_og_plan saves: the leaf scoring of optimize2 under OG_SHANNON at a late decision of a baseline
episode, with the base the leaves of a tree share (k_og_tree_base + k_og_tree_cost, the default) and with k_og_cost on every
materialised leaf (DRLGX_OG_TREE_SHARED=0, the path that existed before).

Two VecExplorationEnv of the 40 m map with the same seeds - one created under the switch - are driven through the same baseline
decisions (OG_SHANNON plans, followed for --steps actions each; the two paths give the same bits, so the episodes are the same), then
og_plan is called --reps times on each, alternating, in one process and session.  The leaf scoring is the engine's timer 6 (HIP
events around the entropy kernels on the engine's stream), the whole call a pair of events around Engine.og_plan; medians.  Also the
whole call under SLAM_OG_SHANNON on the same state.

--walk N: behind the decisions every env walks N scripted actions (a loop of 1.5 m moves and quarter turns), which lengthens the
trajectories to what a late decision has without growing a tree the engine's max_actions refuses on the way; the timed call then runs
with the largest max_nodes of 0.5, 0.25, ... that is served.

    python scripts/micro/og_plan_shared_vs_unshared.py [--envs 50] [--decisions 24] [--walk 0] [--reps 15] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from drl_graph_exploration_amd import em_baseline  # noqa: E402
from drl_graph_exploration_amd._lib import DrlgxError  # noqa: E402
from drl_graph_exploration_amd.vecenv import VecExplorationEnv  # noqa: E402


def make_env(n, shared):
    if not shared:
        os.environ["DRLGX_OG_TREE_SHARED"] = "0"
    try:
        return VecExplorationEnv(40, n, env_index=list(range(n)), test=True, max_poses=256, n_rollouts=0, algorithm=2)
    finally:
        os.environ.pop("DRLGX_OG_TREE_SHARED", None)


def drive(env, limit, steps):
    """Up to `limit` baseline decisions (plan, follow); returns (decisions followed, whether a plan was refused).  Late in an
    episode a tree can grow deeper than the engine's max_actions, which refuses the call (DRLGX_E_CAPACITY), under any algorithm."""
    env.engine.set_env_obstacles(True)
    for d in range(limit):
        try:
            plan, n_act, result = env.em_plan(em_baseline.MAX_NODES, 2048, safe_distance=em_baseline.PLANNER_SAFE_DISTANCE)
        except DrlgxError:
            return d, True
        env.follow(plan, n_act, result, steps=steps)
    return limit, False


def timed_plan(env, sel, start, alg, alpha=0.5):
    """(leaf-scoring ms from the engine's timer 6, whole-call ms from events, outputs) of one og_plan."""
    e = env.engine
    e.timing_read()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    o = e.og_plan(sel, start, 2048, alg, alpha)
    b.record()
    torch.cuda.synchronize(env.device)
    return e.timing_read()["t6"][0], a.elapsed_time(b), o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=50)
    ap.add_argument("--decisions", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--walk", type=int, default=0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.envs
    probe = make_env(n, True)  # the latest of the first --decisions decisions at which the whole vector can still be planned
    done, refused = drive(probe, args.decisions, args.steps)
    probe.close()
    decisions = done - 1 if refused else done
    assert decisions >= 1
    envs = {"shared": make_env(n, True), "unshared": make_env(n, False)}
    for env in envs.values():
        assert drive(env, decisions, args.steps) == (decisions, False)
        loop = [(1.5, 0.0, 0.0)] * 3 + [(0.0, 0.0, math.pi / 2)]
        for k in range(args.walk):
            env.engine.step(torch.tensor([loop[k % len(loop)]] * n, dtype=torch.float64, device=env.device))
        assert env.engine.status() == 0
        env.engine.set_sampler_obstacles(True)
    sel = torch.arange(n, dtype=torch.int32, device=envs["shared"].device)
    start = envs["shared"]._halton_next.clone()
    max_nodes = em_baseline.MAX_NODES
    while True:  # the largest max_nodes whose trees the engine serves from this state
        try:
            for env in envs.values():
                env.engine.set_sampler_parameter(max_nodes, em_baseline.PLANNER_SAFE_DISTANCE)
                env.engine.og_plan(sel, start, 2048, 2)
            break
        except DrlgxError:
            max_nodes /= 2
    for env in envs.values():
        env.engine.timing_enable(True)
    t = {k: dict(score=[], call=[], call3=[]) for k in envs}
    outs = {}
    for rep in range(args.reps + 2):  # (two warm-up rounds: allocations, first launches)
        for k, env in envs.items():
            s, c, o = timed_plan(env, sel, start, 2)
            _, c3, _ = timed_plan(env, sel, start, 3)
            outs[k] = o
            if rep >= 2:
                t[k]["score"].append(s); t[k]["call"].append(c); t[k]["call3"].append(c3)
    same = all(torch.equal(outs["shared"][k], outs["unshared"][k]) for k in ("plan", "n_actions", "cost", "n_leaves", "halton_next"))
    lv = envs["shared"].engine.em_plan_leaves()
    P = envs["shared"].engine.counts_dev()[:, 0].cpu().numpy()
    K = lv["n_actions"].cpu().numpy()
    nl = outs["shared"]["n_leaves"].cpu().numpy()
    med = lambda v: statistics.median(v)  # noqa: E731
    lines = [
        "# scripts/micro/og_plan_shared_vs_unshared.py on an MI355X: %d envs of the 40 m map after %d baseline decisions of %d steps" % (n, decisions, args.steps)
        + (" and %d scripted actions, max_nodes %g" % (args.walk, max_nodes) if args.walk else ""),
        "# (OG_SHANNON%s), one process and session, the two engines alternating, median of %d calls (min - max)."
        % ("; the plan after one more decision is refused: a tree deeper than max_actions" if refused else "", args.reps),
        "state: poses per env mean %.1f (min %d, max %d); leaves per tree mean %.1f (min %d, max %d), %d leaves in all; actions per leaf mean %.2f (max %d)"
        % (P.mean(), P.min(), P.max(), nl.mean(), nl.min(), nl.max(), int(nl.sum()), K.mean(), K.max()),
        "plans, costs, leaf counts and Halton indices of the two paths bit-equal: %s" % same,
    ]
    for k in ("shared", "unshared"):
        lines.append("%-9s leaf scoring (timer 6) %.4f ms (%.4f - %.4f)   whole og_plan, algorithm 2: %.3f ms (%.3f - %.3f)   algorithm 3: %.2f ms (%.2f - %.2f)"
                     % (k, med(t[k]["score"]), min(t[k]["score"]), max(t[k]["score"]), med(t[k]["call"]), min(t[k]["call"]), max(t[k]["call"]),
                        med(t[k]["call3"]), min(t[k]["call3"]), max(t[k]["call3"])))
    lines.append("shared / unshared leaf scoring: %.3f" % (med(t["shared"]["score"]) / med(t["unshared"]["score"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
