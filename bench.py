#!/usr/bin/env python
"""bench.py — env-steps/sec of the MI355X belief-step hot path (BASELINE.json metric).

Workload (BASELINE.json configs[1]): 256 parallel environments per GPU, 40x40 m map
(V = 1600 virtual cells), 100 ground-truth landmarks, every env warmed with a fixed motion script to a
~64-node pose/landmark graph (36 poses + the landmarks seen so far) and snapshotted on the device.
One timed "step" = one belief update (SS2D.simulate(core=True): move, 2 noisy measure calls, factor
append, iSAM2-policy SLAM solve + all block marginals, occupancy + virtual-map rebuild, utility
reductions) for all 256 envs, starting from the snapshot (the device-side restore is inside the timed
region so the graph size stays at the quoted ~64 nodes).  All inputs are resident in HBM.

Multi-GPU: one process per GPU (torch.distributed / RCCL), independent environments per rank, no
data-path collective in the belief step (weak scaling); time = max over ranks.  `--gpus N` without a launcher
re-executes itself under `torch.distributed.run` with N ranks; under a launcher WORLD_SIZE must equal --gpus.
The only exchange of the path is the policy gradient: the `train_allreduce` section of the --full line times the
64-graph DQN step with the flat gradient all-reduce (RCCL over xGMI), the collective alone, and the belief steps
sustained while that training runs on a second stream (BASELINE.json configs[3]).

Output: ONE JSON line on rank 0 (see the driver contract).  A plain run sets up, warms up, times --steps steps and
prints the headline figure (`value`, `ms_per_step`).  `--full` adds, after the timed steps, `roofline` for the
time-dominant kernel (per-kernel HIP-event timing on the engine stream), `kernels` for all three, the
`train_allreduce` section, the secondary sections and `cpu_baseline` = the CPU oracle ("port") timed
single-threaded on the same box.  `--dump-outputs DIR` writes the belief the last timed step computed (float64 .npy).
"""
import argparse
import json
import math
import os
import sys
import time

# (multi-process GPU work on this platform needs dmabuf IPC - RCCL fails with hipIpcGetMemHandle otherwise; set before HIP loads)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_ENVS = 256
MAP = 40
NUM_LM = 100
WARM_SCRIPT = [(1, 1, math.pi / 2)] * 4 + [(2, 0, 0), (2, 0, 0), (0, 0, 0.6)] * 10 + [(2, 0, 0)]  # -> 36 poses
STEP_ACTION = (2.0, 0.0, 0.0)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def algorithmic_bytes(P, L, M, V):
    """SURVEY.md §8(d) per-env-step algorithmic bytes (fp64, perfect on-chip reuse)."""
    n = 3 * P + 2 * L
    cov = 96 * P + 41 * V + 16          # covariance propagation + utility (a9 + a10)
    occ = 24 * P + 16 * L + 8 * V       # occupancy rebuild (a7/a8)
    slam = 56 * P + 40 * M + 8 * n + 72 * P + 32 * L  # factors, state, marginal blocks (a5/a6)
    # GT landmarks + poses (a2-a4).  (The two mt19937 streams the simulator also reads and writes every step - 10 KB - are
    # an implementation cost, not in the survey's count: left out, so that `achieved` is the contract's figure.)
    sim = 16 * NUM_LM + 32 * 2
    return {"map": cov + occ, "slam": slam, "sim": sim}


def make_engine(device_index, seed0, max_poses=41):
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    cfg = default_config(MAP, num_landmarks=NUM_LM, max_poses=max_poses, max_landmarks=100, max_factors=12 * max_poses + 20,
                         max_snapshots=1)
    eng = Engine(cfg, N_ENVS, 4096, device=device_index)  # rollout instances of the look-ahead (VecExplorationEnv's default: min(n_envs (max_landmarks + 1), 4096))
    ids = np.arange(N_ENVS)
    eng.reset(ids, seed0 + ids, los=seed0 + ids)
    for act in WARM_SCRIPT:
        eng.step(torch.tensor([act] * N_ENVS, dtype=torch.float64, device=eng.device))
    eng.check_status()
    eng.snapshot(0)
    return eng, cfg


def cpu_baseline(budget_s=12.0):
    """The CPU oracle (a port of the reference arithmetic, not the reference binary) on ONE host thread:
    same config, envs warmed with the same script, belief updates timed on fresh clones."""
    from oracle import oracle as O
    ocfg = O.default_config(MAP, num_landmarks=NUM_LM)
    sims = []
    t_prep = time.time()
    for lo in range(4):
        s = O.OracleSim(ocfg, lo, lo)
        for act in WARM_SCRIPT:
            s.simulate(act)
        sims.append(s)
        if time.time() - t_prep > budget_s:
            break
    n = 0
    t = 0.0
    while t < budget_s:
        for s in sims:
            c = s.clone()
            t0 = time.perf_counter()
            c.simulate(STEP_ACTION)
            t += time.perf_counter() - t0
            n += 1
    return {"value": n / t, "unit": "env-steps/sec", "cores": 1, "kind": "port",
            "sample": "%d belief updates (SS2D.simulate) on %d seeded envs at 36 poses / ~%d landmarks, %.1f s of CPU work, "
                      "single thread, oracle/drlgx_oracle.cpp -O3" % (n, len(sims), sims[0].num_landmarks(), t),
            "host_cores_available": os.cpu_count()}


def _cpu_worker(args):
    """One process of the all-cores CPU figure: the single-thread measurement on its own seeded env."""
    lo, budget_s = args
    from oracle import oracle as O
    ocfg = O.default_config(MAP, num_landmarks=NUM_LM)
    s = O.OracleSim(ocfg, lo, lo)
    for act in WARM_SCRIPT:
        s.simulate(act)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s:
        s.clone().simulate(STEP_ACTION)
        n += 1
    return n, time.perf_counter() - t0


def cpu_baseline_all_cores(budget_s=6.0, max_procs=None):
    """the same oracle with independent environments sharded over host processes (the CPU
    analogue of the env-parallel GPU path), every process timing its own clone-and-step loop.  Plain subprocesses with a
    timeout: a failure yields an error entry, never a hung benchmark."""
    import subprocess
    # every host core the process may run on (DRLGX_BENCH_MAX_PROCS caps it, and the cap is named in `sample`)
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cap = max_procs if max_procs is not None else int(os.environ.get("DRLGX_BENCH_MAX_PROCS", "0")) or avail
    procs = max(1, min(cap, avail))
    env = dict(os.environ, OMP_NUM_THREADS="1", HIP_VISIBLE_DEVICES="")
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(lo), str(budget_s)], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for lo in range(procs)]
    rate, ok = 0.0, 0
    deadline = time.time() + budget_s + 90.0
    for k in kids:
        try:
            out, _ = k.communicate(timeout=max(1.0, deadline - time.time()))
            n, t = out.strip().split()[-2:]
            rate += float(n) / float(t)
            ok += 1
        except Exception:  # noqa: BLE001 - timeout, crash or unparsable output: skip this process
            k.kill()
    if ok == 0:
        return {"error": "no CPU worker finished"}
    return {"value": rate, "unit": "env-steps/sec", "cores": ok, "kind": "port", "host_cores_available": avail,
            "sample": "%d processes (of %d cores available%s) x %.0f s of clone-and-step on one seeded env each (36 poses), "
                      "oracle/drlgx_oracle.cpp -O3" % (ok, avail, "" if procs == avail else ", capped at %d" % procs, budget_s)}


MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: f32-input MFMA = the fp32 vector rate


def policy_bench(eng, dev, iters=10):
    """Secondary measurements on the same engine (NOT the headline metric): the decision-side path (graph export,
    line plans + look-ahead rewards for every frontier, GCN forward over the 256-graph batch) and one DQN train step
    (GCN forward + backward on a 64-graph batch). The GCN is fp32 on f32-input MFMA (`v_mfma_f32_16x16x4_f32` /
    `v_mfma_f32_32x32x2_f32`)."""
    from drl_graph_exploration_amd.networks import GCN, GraphData

    def timed(fn, n=iters):
        # the better of two runs of n calls: a single run now and then catches a one-off host stall of tens of milliseconds
        # (allocator / page-in behind the CPU-surrogate section) that multiplies a sub-millisecond figure
        fn()
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            best = dt if best is None else min(best, dt)
        return best

    torch.manual_seed(0)
    model = GCN().to(dev)
    # the look-ahead appends up to max_actions poses to the 37-pose trajectories: its own engine with room for them
    # (the kernels are picked per launch from the actual trajectory lengths, not from this capacity)
    eng.close()
    eng, _ = make_engine(dev.index or 0, 0, max_poses=64)
    eng.restore(0)
    out = {}
    g = eng.graph()
    N, E = int(g["x"].shape[0]), int(g["edge_index"].shape[1])
    nfr = g["n_frontier"].long()
    cand_env = torch.repeat_interleave(torch.arange(N_ENVS, device=dev), nfr).to(torch.int32)
    first = torch.cumsum(nfr, 0) - nfr
    fidx = torch.arange(cand_env.numel(), device=dev) - first[cand_env.long()]
    goals = g["frontier_xy"][cand_env.long(), fidx].contiguous()
    data = GraphData(g["x"], g["edge_index"], g["edge_attr"], g["batch"], g["node_off"], g["edge_off"], g["max_graph_edges"])
    out["graph_nodes"], out["graph_edges"], out["candidates"] = N, E, int(cand_env.numel())
    out["graph_export_ms"] = timed(lambda: eng.graph()) * 1e3
    acts, nact = eng.line_plan(cand_env, goals)
    out["line_plan_ms"] = timed(lambda: eng.line_plan(cand_env, goals)) * 1e3
    out["lookahead_ms"] = timed(lambda: eng.lookahead(cand_env, acts, nact, max_n_actions=int(nact.max())), n=3) * 1e3
    eng.check_status()  # no rollout ran out of capacity
    out["rollout_steps"] = int(nact.sum())
    with torch.no_grad():
        t_f = timed(lambda: model(data, 0.0))
    flops_f = 2.0 * N * (5 * 1000 + 1000 * 1000 + 1000) + 2.0 * 2 * (E + N) * 1000  # GEMMs + two aggregations
    out["gcn_forward_ms"] = t_f * 1e3
    out["gcn_forward_TFLOPs"] = flops_f / t_f / 1e12
    # the PyG-CPU surrogate beside it: the plain-PyTorch restatement of Networks.GCN.forward
    # (oracle/gcn_ref.py: x @ W + index_add_) on the SAME 256-graph batch on the host, and on one graph of it (the reference
    # evaluates one graph per decision); the only reference-measured policy number is quoted beside, not as a ratio
    try:
        from oracle import gcn_ref
        params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        xc, eic, eac = g["x"].cpu(), g["edge_index"].cpu(), g["edge_attr"].cpu()
        n1, e1 = int(g["node_off"][1]), int(g["edge_off"][1])

        def cpu_timed(fn, budget=4.0):
            fn()
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < budget:
                fn()
                n += 1
            return (time.perf_counter() - t0) / n, n
        with torch.no_grad():
            t_b, n_b = cpu_timed(lambda: gcn_ref.gcn_forward(params, xc, eic, eac))
            t_1, n_1 = cpu_timed(lambda: gcn_ref.gcn_forward(params, xc[:n1], eic[:, :e1], eac[:e1]), budget=2.0)
        out["cpu_baseline"] = {"kind": "port", "what": "oracle/gcn_ref.py (plain PyTorch CPU restatement of GCNConv(improved=True) x 2 + Linear)",
                               "torch_threads": torch.get_num_threads(), "batch_forward_ms": t_b * 1e3, "batch_forwards_timed": n_b,
                               "single_graph_forward_ms": t_1 * 1e3, "single_graph_nodes": n1,
                               "gpu_over_cpu_batch_forward": t_b / t_f,
                               "reference_published": "7.25 ms mean per single-graph GCN forward (data/test_result/40_DQN_GCN.csv, timer at "
                                                      "scripts/test.py:109-116; authors' PC, GPU not stated) - other hardware, reported beside"}
    except Exception as ex:  # noqa: BLE001 - the oracle is optional for the bench line
        out["cpu_baseline"] = {"error": repr(ex)}
    out["decisions_per_sec"] = N_ENVS / (out["graph_export_ms"] + out["line_plan_ms"] + out["lookahead_ms"] + t_f * 1e3) * 1e3
    # train step: 64-graph minibatch (the first 64 envs' graphs)
    n64 = int(g["node_off"][64])
    e64 = int(g["edge_off"][64])
    d64 = GraphData(g["x"][:n64], g["edge_index"][:, :e64], g["edge_attr"][:e64], g["batch"][:n64], g["node_off"][:65], g["edge_off"][:65], g["max_graph_edges"])
    train_step = make_train_step(model, d64, dev)
    t_t = timed(train_step)
    flops_t = 3 * (2.0 * n64 * (5 * 1000 + 1000 * 1000 + 1000)) + 2.0 * 4 * (e64 + n64) * 1000
    out["train_step_ms"] = t_t * 1e3
    out["train_step_nodes"] = n64
    out["train_step_TFLOPs"] = flops_t / t_t / 1e12
    out["mfma_f32_peak_TFLOPs"] = MFMA_F32_PEAK_TFLOPS
    out["gcn_forward_frac_mfma_peak"] = out["gcn_forward_TFLOPs"] / MFMA_F32_PEAK_TFLOPS
    eng.close()
    return out


def dqn_loop_bench(device_index, n_envs=256, iters=8):
    """BASELINE config 2 as a secondary figure: wall-clock rate of the whole DQN loop (`DeepQ.running`: graph export,
    look-ahead rewards of every frontier, policy forward, env step, replay, one 64-graph train step per ENVIRONMENT step
    like the reference - n_envs per vector step -, episode resets), in the reference's unit - RL iterations (decisions)
    per second."""
    import tempfile
    from drl_graph_exploration_amd.networks import GCN
    from drl_graph_exploration_amd.policy import DeepQ
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    dev = torch.device("cuda", device_index)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        dq = DeepQ("bench/", "GCN", data_root=tmp)
        dq.OBSERVE, dq.epoch = n_envs, n_envs * 3  # warm-up: 3 vector steps, training from the 2nd
        pol, tgt = GCN().to(dev), GCN().to(dev)
        tgt.load_state_dict(pol.state_dict())
        env = VecExplorationEnv(MAP, n_envs, env_index=0, test=True, device=device_index)  # (construction is not timed)
        dq.running(pol, tgt, test=True, env=env)
        dq.epoch = n_envs * iters
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dq.running(pol, tgt, test=True, env=env)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        env.close()
    return {"workload": "DeepQ.running, %d envs in lock-step, 40 m map, one train step (64 graphs) per environment step" % n_envs,
            "ms_per_vector_step": dt / iters * 1e3, "rl_iterations_per_sec": n_envs * iters / dt,
            "reference_published": "~3.8 RL iterations/s (A2C+GCN, authors' PC; BASELINE.md) - other hardware, reported beside"}


def a2c_loop_bench(device_index, n_envs=256, iters=40):
    """The configuration BASELINE.md's only published rate is quoted on (A2C + GCN, ~3.8 RL iterations/s on the authors' PC),
    as a secondary figure: wall-clock rate of `A2C.running` (graph export, look-ahead rewards, actor and critic forward,
    sampled actions, env step, and one actor-critic update over all n_envs x nstep transitions every nstep = 40 vector
    steps like the reference), in RL iterations (decisions) per second."""
    import tempfile
    from drl_graph_exploration_amd.networks import PolicyGCN, ValueGCN
    from drl_graph_exploration_amd.policy import A2C
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    dev = torch.device("cuda", device_index)
    torch.manual_seed(0)
    np.random.seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        a2c = A2C("bench_a2c/", data_root=tmp)
        actor, critic = PolicyGCN().to(dev), ValueGCN().to(dev)
        env = VecExplorationEnv(MAP, n_envs, env_index=0, test=True, device=device_index)
        a2c.epoch, a2c.nstep = n_envs * 2, 2  # warm-up: two vector steps and one small update (first-use allocations)
        a2c.running(actor, critic, test=True, env=env)
        a2c.epoch, a2c.nstep = n_envs * iters, 40  # 40 vector steps: exactly one update over all of them in the timed region
        a2c.buffer.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a2c.running(actor, critic, test=True, env=env)  # (vector steps 3 .. 42 of the episodes: a second pass would time later, longer trajectories)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        env.close()
    return {"workload": "A2C.running, %d envs in lock-step, 40 m map, %d vector steps with one update over %d transitions" % (
                n_envs, iters, n_envs * iters),
            "ms_per_vector_step": dt / iters * 1e3, "rl_iterations_per_sec": n_envs * iters / dt,
            "reference_published": "~3.8 RL iterations/s (A2C+GCN, authors' PC; BASELINE.md) - other hardware, reported beside"}


def config5_bench(device_index, n_envs=256, warm=108, timed=10):
    """BASELINE config 5 scale as a secondary figure: 50 m map, 500 landmarks, graphs grown by a fixed motion loop to
    ~110 poses / ~95 landmarks; per-stage kernels (more landmarks than the fused kernels sweep in LDS).  The timed region is one
    whole cycle of the iSAM2 counter - ten consecutive updates, one of them the relinearising 10th - so that `ms_per_step` is what
    a trajectory pays on average; a second pass with events gives the stage kernels' rows, incremental and relinearising updates
    apart (SLAM stage: k_slam_arrow - between relinearisations the rank-k update of k_inc.hip with the covariance panel in HBM / L2,
    ONE walk over it per batch of up to 32 re-observed landmarks)."""
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    cfg = default_config(50, num_landmarks=500, max_poses=127, max_landmarks=127, max_factors=3800)
    eng = Engine(cfg, n_envs, 0, device_index)
    rng = np.random.RandomState(0)
    starts = np.stack([rng.uniform(-12, 12, n_envs), rng.uniform(-12, 12, n_envs), rng.uniform(-3, 3, n_envs)], 1)
    eng.reset(np.arange(n_envs), np.arange(n_envs), starts=starts)
    loop = [(2, 0, 0)] * 3 + [(0, 0, math.pi / 2)] + [(2, 0, 0)] * 2 + [(0.7, 0, 0.4)]
    odoms = [torch.tensor([a] * n_envs, dtype=torch.float64, device=eng.device) for a in loop]
    for s in range(warm):
        eng.step(odoms[s % len(loop)])
    eng.synchronize()
    eng.check_status()
    eng.snapshot(0)
    c = eng.counts_dev().cpu().numpy()
    t0 = time.perf_counter()
    for s in range(timed):
        eng.step(odoms[(warm + s) % len(loop)])
    eng.synchronize()
    dt = (time.perf_counter() - t0) / timed
    eng.check_status()
    # the same ten updates again from the snapshot, one at a time with events around the stage kernels
    eng.restore(0)
    eng.timing_enable(2)
    rows = {"incremental": {"sim": [], "slam": [], "map": []}, "relinearising": {"sim": [], "slam": [], "map": []}}
    V = eng.rows * eng.cols
    for s in range(timed):
        eng.inc_stats(reset=True)
        eng.timing_read()
        eng.step(odoms[(warm + s) % len(loop)])
        eng.synchronize()
        tm = eng.timing_read()
        inc, full = eng.inc_stats(reset=True)
        ev = tm["t7"][0] / max(tm["t7"][1], 1) * 1e3
        kind = "incremental" if inc >= full else "relinearising"
        for k in ("sim", "slam", "map"):
            if tm[k][1]:
                rows[kind][k].append(tm[k][0] / tm[k][1] * 1e3 - ev)
    eng.timing_enable(False)
    eng.check_status()
    eng.close()
    P, L, M = float(c[:, 0].mean()) + timed / 2.0, float(c[:, 1].mean()), float(c[:, 2].mean())
    ab = algorithmic_bytes(P, L, M, V)
    # what the incremental update keeps INSTEAD of recomputing: the covariance panel Sigma[:, active], read and written once per walk
    panel_bytes = (3 * P + 2 * L) * (3 + 2 * L) * 8
    kernels = {}
    for kind, st in rows.items():
        for k, v in st.items():
            if not v:
                continue
            us = float(np.mean(v))
            ent = {"avg_us_per_launch": us, "launches": len(v), "algorithmic_bytes_per_launch": ab[k] * n_envs,
                   "achieved_GBs": ab[k] * n_envs / (us * 1e-6) / 1e9, "frac_hbm_peak": ab[k] * n_envs / (us * 1e-6) / 1e9 / HBM_PEAK_GBS}
            if k == "slam" and kind == "incremental":
                ent["panel_bytes_read_and_written_per_walk"] = 2 * panel_bytes * n_envs
                ent["panel_traffic_frac_hbm_peak_at_one_walk"] = 2 * panel_bytes * n_envs / (us * 1e-6) / 1e9 / HBM_PEAK_GBS
            kernels["%s_%s" % (k, kind)] = ent
    return {"workload": "50x50 map (V=%d), 500 landmarks, %d envs; %d consecutive updates (one relinearising)" % (V, n_envs, timed),
            "poses": float(c[:, 0].mean()), "landmarks": L, "factors": M, "ms_per_step": dt * 1e3,
            "env_steps_per_sec": n_envs / dt, "kernels": kernels}


def update_cycle_bench(device_index, reps=10, steps=10):
    """The headline step is ONE belief update from the snapshot (update #37 of the iSAM2 counter: no relinearisation due, so
    the incremental rank-k update serves it).  This section times what a trajectory pays on average: `steps` consecutive
    updates from the snapshot (the graphs grow from 37 to 46 poses; one of them is a 10th update, where the envs whose
    deltas crossed the threshold relinearise and take the full solve), restore not included.  (Its own engine with room
    for the ten poses; the kernels follow the trajectory lengths, not the capacity.)"""
    eng, _ = make_engine(device_index, 0, max_poses=64)
    odom = torch.tensor([STEP_ACTION] * N_ENVS, dtype=torch.float64, device=eng.device)
    eng.inc_stats(reset=True)
    eng.restore(0)
    for _ in range(steps):
        eng.step(odom)
    eng.synchronize()
    inc, full = eng.inc_stats(reset=True)
    t = 0.0
    for _ in range(reps):
        eng.restore(0)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step(odom)
        eng.synchronize()
        t += time.perf_counter() - t0
    eng.check_status()
    eng.close()
    return {"workload": "%d consecutive belief updates from the snapshot (37 -> %d poses), restore outside the timed region" % (steps, 36 + steps),
            "ms_per_step": t / (reps * steps) * 1e3, "env_steps_per_sec": N_ENVS * reps * steps / t,
            "slam_updates_incremental": inc, "slam_updates_full_solve": full}


def capacity_bench(device_index, steps=100):
    """The headline loop on an engine created with the DEFAULT pose capacity of the vectorised env (max_poses = 256: what
    DeepQ.running / A2C.running / evaluation use) instead of the bench's 41: the kernels size their per-pose LDS tables and the
    instance copies with the trajectory lengths, not with the capacity."""
    eng, _ = make_engine(device_index, 0, max_poses=256)
    odom = torch.tensor([STEP_ACTION] * N_ENVS, dtype=torch.float64, device=eng.device)
    for _ in range(10):
        eng.restore(0); eng.step(odom)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.restore(0); eng.step(odom)
    eng.synchronize()
    dt = (time.perf_counter() - t0) / steps
    eng.check_status()
    eng.close()
    return {"workload": "the headline loop on an engine with max_poses = 256", "ms_per_step": dt * 1e3, "env_steps_per_sec": N_ENVS / dt}


def full_fill_bench(device_index, n_envs=2048, steps=40):
    """The headline workload with EIGHT workgroups per CU's worth of instances (2 048 envs on one GPU): the per-launch
    figure at 256 envs is the latency of the slowest instance; here the workgroups are dispatched as CUs free up, so the
    launch lasts ~8 average instances - the throughput the step reaches when there are more belief states than CUs (more
    envs per GPU; the look-ahead's rollouts).  Same state (36 poses), same restore + step loop, fused kernel events."""
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    cfg = default_config(MAP, num_landmarks=NUM_LM, max_poses=41, max_landmarks=100, max_factors=12 * 41 + 20, max_snapshots=1)
    eng = Engine(cfg, n_envs, 0, device=device_index)
    ids = np.arange(n_envs)
    eng.reset(ids, ids, los=ids)
    for act in WARM_SCRIPT:
        eng.step(torch.tensor([act] * n_envs, dtype=torch.float64, device=eng.device))
    eng.check_status()
    eng.snapshot(0)
    odom = torch.tensor([STEP_ACTION] * n_envs, dtype=torch.float64, device=eng.device)
    for _ in range(5):
        eng.restore(0); eng.step(odom)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.restore(0); eng.step(odom)
    eng.synchronize()
    dt = (time.perf_counter() - t0) / steps
    eng.timing_enable(True); eng.timing_read()
    for _ in range(steps):
        eng.restore(0); eng.step(odom)
    tm = eng.timing_read()
    eng.timing_enable(2)  # ... and as the three stage kernels, for the map stage's own figure at this fill
    for _ in range(steps):
        eng.restore(0); eng.step(odom)
    tm3 = eng.timing_read()
    eng.check_status()
    eng_counts = eng.counts_dev().cpu().numpy()[:, :3].astype(np.float64).mean(axis=0)  # poses, landmarks, factors
    V = eng.rows * eng.cols
    eng.close()
    step_us = tm["step"][0] * 1e3 / max(tm["step"][1], 1)
    c = eng_counts
    ab = algorithmic_bytes(c[0], c[1], c[2], V)
    bytes_per_env = sum(ab.values())
    map_us = tm3["map"][0] * 1e3 / max(tm3["map"][1], 1)
    return {"workload": "configs[1]'s state with %d envs on one GPU (8 workgroups per CU in one launch)" % n_envs,
            "ms_per_step": dt * 1e3, "env_steps_per_sec": n_envs / dt, "k_step_us_per_launch_incl_event_overhead": step_us,
            "k_step_env_steps_per_sec": n_envs / (step_us * 1e-6),
            "k_step_frac_hbm_peak": bytes_per_env * n_envs / (step_us * 1e-6) / 8e12,
            "k_map_us_per_launch_incl_event_overhead": map_us, "k_map_frac_hbm_peak": ab["map"] * n_envs / (map_us * 1e-6) / 8e12}


BELIEF_STEP_SOURCES = ("drlgx_dev.h", "drlgx_fields.h", "k_sim.hip", "k_slam.hip", "k_slam_arrow.hip", "k_inc.hip", "k_map.hip", "k_step.hip",
                       "drlgx_engine.cpp")


def csrc_digest():
    """sha1 over the sources of the belief-step kernels (the fused step's translation unit and the engine): ties a PMC
    counter file to the tree it was measured on (no .git on the GPU box)."""
    import hashlib
    h = hashlib.sha1()
    for name in BELIEF_STEP_SOURCES:
        h.update(name.encode())
        h.update(open(os.path.join(ROOT, "drl_graph_exploration_amd", "csrc", name), "rb").read())
    return h.hexdigest()


def spawn_command(args_list, n):
    """The launcher the driver itself uses for N > 1 (one rank per GPU, rendezvous on 127.0.0.1)."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(args_list)


def make_train_step(model, d64, dev, split=False):
    """The reference's DQN update on one 64-graph mini-batch as the product's trainer issues it (`DeepQ._train_minibatches`):
    the graphs live in a device replay pool whose per-graph normalisation / CSRs / AX were cached when they were stored; per
    update ONE collation from that cache + the TD targets (drlgx_dqn_prepare), trunk forward with dropout + float64 cost +
    gradient + trunk backward (drlgx_dqn_forward_backward), [gradient all-reduce over the ranks,] clamp + Adam.  Synthetic
    rewards, one action node per graph, next state = the same graph (its cached target read-out is gathered and used)."""
    import random
    import tempfile
    from drl_graph_exploration_amd.networks import PoolRef, ReplayPool
    from drl_graph_exploration_amd.optim import FusedAdam
    from drl_graph_exploration_amd.policy import DeepQ
    dq = DeepQ("bench_train/", "GCN", data_root=tempfile.mkdtemp(prefix="drlgx_bench_"))
    opt = FusedAdam(model.parameters(), lr=1e-5, grad_clamp=dq.max_grad_norm)
    no, eo = d64.node_off.cpu().numpy().astype(np.int64), d64.edge_off.cpu().numpy().astype(np.int64)
    B = len(no) - 1
    pool = ReplayPool(dev, 2, int(no[-1]), max(int(eo[-1]), 1), cache_csr=True)
    slot = pool.put({"x": d64.x, "edge_index": d64.edge_index, "edge_attr": d64.edge_attr, "node_off_h": no, "edge_off_h": eo,
                     "node_off": d64.node_off, "edge_off": d64.edge_off})
    assert pool.csr_ok[slot]
    rng = np.random.RandomState(0)
    for i in range(B):
        ref = PoolRef(pool, slot, i)
        dq.buffer.append((ref, ref.num_nodes - 1, float(rng.randn()), ref, False, 1))
    dq.BATCH = B
    sample, random.sample = random.sample, (lambda pop, k: list(range(k)))  # the mini-batch = the 64 graphs in order
    try:
        prepared, _ = dq._prepare_updates(1, dev, model)  # (evaluates the target read-out of the stored export once: not timed)
    finally:
        random.sample = sample
    pr = prepared[0]
    assert pr["csr"] and pr["N"] == int(no[-1])
    W1, _, _, _, Wf, _ = model.trunk_parameters()
    dims = (int(W1.shape[0]), int(W1.shape[1]), int(Wf.shape[0]))
    model.train()

    def begin():
        return dq._fused_forward_backward(pr, dq._fused_prepare(pr, dev, dims), dev, model, opt)
    if split:  # (begin: collation / targets / forward / cost / backward + the gradient exchange issued; end: wait, clamp + Adam)
        return begin, dq._train_end
    return lambda: dq._train_end(begin())


def train_allreduce_bench(eng, dev, dist, world, iters=20, env_steps_per_iter=8):
    """BASELINE.json configs[3]: the exchange step of the path.  Every rank runs the reference's DQN update on a 64-graph
    batch of its own environments (GCN forward + backward through the HIP kernels, ONE flat all-reduce of the 1 008 001
    gradient elements over RCCL, element-wise clamp, Adam).  Three bracketed timings (barrier + synchronize on both
    sides, max over ranks): the train step, the collective alone, and train steps on a second stream while the belief
    steps keep running on the engine's stream (the overlap SURVEY.md section 5 asks for)."""
    from drl_graph_exploration_amd.networks import GCN, GraphData
    from drl_graph_exploration_amd.policy import allreduce_gradients, broadcast_parameters
    torch.manual_seed(0)
    model = GCN().to(dev)
    broadcast_parameters(model)
    eng.restore(0)
    g = eng.graph()
    n64, e64 = int(g["node_off"][64]), int(g["edge_off"][64])
    d64 = GraphData(g["x"][:n64].clone(), g["edge_index"][:, :e64].clone(), g["edge_attr"][:e64].clone(), g["batch"][:n64].clone(),
                    g["node_off"][:65].clone(), g["edge_off"][:65].clone(), g["max_graph_edges"])
    odom = torch.tensor([STEP_ACTION] * N_ENVS, dtype=torch.float64, device=dev)
    n_param = sum(p.numel() for p in model.parameters())
    flat = torch.zeros(n_param, dtype=torch.float32, device=dev)
    train_step = make_train_step(model, d64, dev)

    def bracket(fn, n):
        for _ in range(3):
            fn()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt / n

    t_train = bracket(train_step, iters)
    t_coll = bracket((lambda: dist.all_reduce(flat)) if dist is not None else (lambda: None), iters)
    # the trainer's own loop shape (DeepQ._train_minibatches): the next mini-batch is collated between an update's backward
    # pass and its Adam step, i.e. while that update's all-reduce travels (stand-in for the collation: a copy of the batch)
    begin, end = make_train_step(model, d64, dev, split=True)

    def pipelined():
        h = begin()
        _ = (d64.x.clone(), d64.edge_index.clone(), d64.edge_attr.clone())
        end(h)
    t_pipe = bracket(pipelined, iters)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())

    def overlapped():
        with torch.cuda.stream(side):  # the trainer's stream; the engine stays on the current stream
            train_step()
        for _ in range(env_steps_per_iter):
            eng.restore(0)
            eng.step(odom)
        torch.cuda.current_stream().wait_stream(side)
    t_ov = bracket(overlapped, iters)
    eng.check_status()
    return {"workload": "configs[3]: per rank 256 envs + DQN update on 64 graphs (%d nodes), flat fp32 gradient all-reduce of %d "
                        "elements (%.2f MB) per train step" % (n64, n_param, n_param * 4 / 1e6),
            "ranks": world, "backend": (dist.get_backend() if dist is not None else "none"),
            "train_step_ms": t_train * 1e3, "allreduce_ms": t_coll * 1e3 if dist is not None else 0.0,
            "train_step_with_next_batch_collated_under_the_exchange_ms": t_pipe * 1e3,
            "overlapped_iteration_ms": t_ov * 1e3, "env_steps_per_iteration": env_steps_per_iter * N_ENVS,
            "env_steps_per_sec_while_training": env_steps_per_iter * N_ENVS * world / t_ov,
            "train_steps_per_sec": world / t_ov}


def dump_outputs(eng, outdir):
    """`--dump-outputs DIR`: the belief every env holds after the last timed step (snapshot restore + one update) - what a caller
    of SS2D.simulate reads back - as float64 .npy files (under 30 MB for 256 envs).  Per-env lists of different lengths are padded
    to the longest with zeros (landmark keys with -1), so every value is finite; `counts` holds each env's poses, landmarks
    and factors.  Inputs are seeded: two builds given the same arguments can be compared file by file."""
    os.makedirs(outdir, exist_ok=True)
    n = eng.n_envs
    arrays = {"utility": eng.utility(), "metrics": eng.metrics(), "counts": eng.counts_dev()[:, :3]}
    arrays["cov_length"], arrays["cov_angle"] = eng.cov_array()
    arrays = {k: v.double().cpu().numpy() for k, v in arrays.items()}
    per_env = {k: [] for k in ("pose_xyt", "pose_info", "landmark_keys", "landmark_xy", "landmark_info", "landmark_cov_trace",
                               "pose_cov_trace", "vm_prob", "vm_info", "vm_cov_trace")}
    for i in range(n):
        xyt, info = eng.poses(i)
        keys, xy, linfo = eng.landmarks(i)
        lm_tr, ps_tr = eng.cov_traces(i)
        prob, vinfo, vtr, _ = eng.virtual_map(i)
        for k, v in zip(per_env, (xyt, info, keys, xy, linfo, lm_tr, ps_tr, prob, vinfo, vtr)):
            per_env[k].append(np.asarray(v, dtype=np.float64))
    for k, vs in per_env.items():
        a = np.full((n, max(len(v) for v in vs)) + vs[0].shape[1:], -1.0 if k == "landmark_keys" else 0.0)
        for i, v in enumerate(vs):
            a[i, :len(v)] = v
        arrays[k] = a
    for k, a in arrays.items():
        np.save(os.path.join(outdir, k + ".npy"), a)


def full_measurements(args, eng, dev, dist, world, local_rank, one_step, P, L, M, out):
    """`--full`: everything the headline figure does not need, on the same engine after its timed steps - the steps again
    with HIP events around every launch (fused kernel, then the three stage kernels: per-kernel times and rooflines), the
    SLAM path split, the DQN-update / gradient all-reduce section (all ranks: it holds collectives), and on one GPU the
    decision-path, scale and trainer-loop sections and the CPU baselines.  Adds their keys to rank 0's line `out`."""
    # second pass: the same steps with HIP events on the engine stream around every launch (fused belief-step kernel)
    eng.timing_enable(True)
    eng.timing_read()
    for _ in range(args.steps):
        one_step()
    tm_fused = eng.timing_read()
    # third pass: the belief step launched as its three stage kernels, for the per-stage breakdown
    eng.timing_enable(2)
    for _ in range(args.steps):
        one_step()
    tm = eng.timing_read()
    eng.timing_enable(False)
    inc_split = eng.inc_stats(reset=True)  # (all launches so far were the headline update)
    train = None
    if not args.no_train:  # every rank takes part: the section contains collectives
        train = train_allreduce_bench(eng, dev, dist, world)
    if out is None:
        return
    V = eng.rows * eng.cols
    ab = algorithmic_bytes(P + 1, L, M, V)
    kernels = {}
    # an empty event pair is recorded once per step: its duration is the measurement overhead of a span
    ev_over_us = tm["t7"][0] / max(tm["t7"][1], 1) * 1e3
    for name in ("sim", "slam", "map", "copy"):
        ms, n = tm[name]
        if n == 0:
            continue
        avg_us = ms / n * 1e3 - ev_over_us
        b = ab.get(name)
        ent = {"avg_us_per_launch": avg_us, "launches": int(n)}
        if b is not None:
            ent["algorithmic_bytes_per_launch"] = b * N_ENVS
            ent["achieved_GBs"] = b * N_ENVS / (avg_us * 1e-6) / 1e9
            ent["frac_hbm_peak"] = ent["achieved_GBs"] / HBM_PEAK_GBS
        kernels[name] = ent
    # the dominant kernel of the timed region is the fused belief step (simulate + SLAM + map of one instance per
    # workgroup); its algorithmic bytes are the sum of the three stages'
    ev2 = tm_fused["t7"][0] / max(tm_fused["t7"][1], 1) * 1e3
    if tm_fused["step"][1] > 0:
        dom = "step"
        step_us = tm_fused["step"][0] / tm_fused["step"][1] * 1e3 - ev2
        step_bytes = (ab["sim"] + ab["slam"] + ab["map"]) * N_ENVS
        kernels["step"] = {"avg_us_per_launch": step_us, "launches": int(tm_fused["step"][1]),
                           "algorithmic_bytes_per_launch": step_bytes, "achieved_GBs": step_bytes / (step_us * 1e-6) / 1e9,
                           "frac_hbm_peak": step_bytes / (step_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                           "note": "fused kernel used by drlgx_step; sim/slam/map entries are the same work launched as three kernels"}
        if tm_fused["copy"][1] > 0:
            kernels["copy"]["avg_us_per_launch"] = tm_fused["copy"][0] / tm_fused["copy"][1] * 1e3 - ev2
    else:  # capacities beyond the fused kernel
        dom = max(("sim", "slam", "map"), key=lambda k: kernels[k]["avg_us_per_launch"])
    roofline = {"kernel": {"sim": "k_sim_step", "slam": "k_slam", "map": "k_map", "step": "k_step"}[dom], "bound": "hbm",
                "achieved": kernels[dom]["achieved_GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": kernels[dom]["frac_hbm_peak"], "traffic": None,
                "avg_us_per_launch": kernels[dom]["avg_us_per_launch"]}
    # HBM traffic per launch comes from separate rocprofv3 --pmc passes over this same command (counters cannot be
    # read in-process): profiles/pmc_traffic.json holds the corrected per-kernel figures (scripts/rocpd_pmc.py) and
    # the digest of the kernel sources they were measured on - traffic is reported only when that is THIS tree
    roofline["algorithmic_bytes_per_launch"] = kernels[dom]["algorithmic_bytes_per_launch"]
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            pmc = json.load(f)
        if pmc.get("csrc_sha1") == csrc_digest():
            roofline["traffic"] = pmc["kernels"][roofline["kernel"]]["hbm_traffic_bytes_per_launch"]
            roofline["traffic_source"] = ("profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, bytes/launch), "
                                          "measured on kernel sources sha1 %s = this tree" % pmc["csrc_sha1"][:12])
        else:
            roofline["traffic_source"] = "profiles/pmc_traffic.json is from other kernel sources (sha1 %s): not reported" % str(pmc.get("csrc_sha1"))[:12]
    except (OSError, KeyError, ValueError):
        pass
    # second roofline entry, for the bound the SQ counters support: the belief step is neither an HBM nor an MFMA
    # kernel - its waves spend most of their cycles parked on waitcnt / barriers of dependent fp64 chains - so the
    # closest throughput ceiling is VALU instruction issue (one wave64 instruction per SIMD per 4 cycles).  Counters
    # come from profiles/sq_counters.json (scripts/collect_profiles.sh), quoted only for THIS tree's kernel sources
    roofline_issue = None
    try:
        with open(os.path.join(ROOT, "profiles", "sq_counters.json")) as f:
            sq = json.load(f)
        if sq.get("csrc_sha1") == csrc_digest():
            c = sq["kernels"][roofline["kernel"]]
            peak = 256 * 4 * 2.4e9 / 4.0 / 1e9  # G wave64 VALU instructions/s: 1024 SIMDs, 4 cycles each
            ach = c["SQ_INSTS_VALU"] / (roofline["avg_us_per_launch"] * 1e-6) / 1e9
            wc = c["SQ_WAVE_CYCLES"]
            roofline_issue = {
                "kernel": roofline["kernel"], "bound": "valu-issue", "achieved": ach, "peak": peak,
                "unit": "G wave64 VALU instructions/s", "frac": ach / peak,
                "wave_cycle_shares": {"issuing_any": c["SQ_ACTIVE_INST_ANY"] / wc, "issuing_valu": c["SQ_ACTIVE_INST_VALU"] / wc,
                                      "parked_on_waitcnt_or_barrier": c["SQ_WAIT_ANY"] / wc,
                                      "issue_stalled": c["SQ_WAIT_INST_ANY"] / wc},
                "mfma_f64_pipe_busy": c["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024.0 * c["GRBM_GUI_ACTIVE"] / 8.0),
                "valu_instructions_per_wave": c["SQ_INSTS_VALU"] / c["SQ_WAVES"],
                "note": "peak assumes 4 cycles per wave64 VALU instruction, which holds for fp64 only (fp32 / integer "
                        "instructions issue in 2): frac is an upper bound of the issue utilisation",
                "source": "profiles/sq_counters.json (rocprofv3 --pmc SQ_*), kernel sources sha1 %s = this tree" % sq["csrc_sha1"][:12]}
    except (OSError, KeyError, ValueError, ZeroDivisionError):
        pass
    # ... and the same bound for the kernel the north star sets a target for (the covariance-propagation kernel k_map, stand-alone
    # form, 256 instances): its VALU instruction count per launch against the issue rate of 1 024 SIMDs
    roofline_issue_map = None
    try:
        if sq.get("csrc_sha1") == csrc_digest() and "k_map" in sq["kernels"] and "map" in kernels:
            c = sq["kernels"]["k_map"]
            peak = 256 * 4 * 2.4e9 / 4.0 / 1e9
            us = kernels["map"]["avg_us_per_launch"]
            roofline_issue_map = {
                "kernel": "k_map", "bound": "valu-issue", "achieved": c["SQ_INSTS_VALU"] / (us * 1e-6) / 1e9, "peak": peak,
                "unit": "G wave64 VALU instructions/s", "frac": c["SQ_INSTS_VALU"] / (us * 1e-6) / 1e9 / peak,
                "valu_instructions_per_instance": c["SQ_INSTS_VALU"] / N_ENVS,
                "us_of_pure_fp64_issue_per_cu": c["SQ_INSTS_VALU"] / N_ENVS / 4.0 * 4.0 / 2.4e3,
                "avg_us_per_launch": us, "frac_hbm_peak": kernels["map"]["frac_hbm_peak"],
                "wave_cycle_shares": {"issuing_valu": c["SQ_ACTIVE_INST_VALU"] / c["SQ_WAVE_CYCLES"],
                                      "parked_on_waitcnt_or_barrier": c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"]},
                "note": "one workgroup (8 waves, 4 SIMDs) per CU: an instance's VALU instructions / 4 SIMDs x 4 cycles is the time its CU "
                        "needs to ISSUE them if they were all fp64 - the floor of the launch under this instruction count",
                "source": "profiles/sq_counters.json, kernel sources sha1 %s = this tree" % sq["csrc_sha1"][:12]}
    except (NameError, KeyError, ValueError, ZeroDivisionError):
        pass
    out.update({
        "roofline": roofline, "roofline_issue": roofline_issue, "roofline_issue_k_map": roofline_issue_map, "kernels": kernels,
        "event_pair_overhead_us": ev_over_us,
        "slam_path": {"incremental_updates": inc_split[0], "full_solves": inc_split[1],
                      "note": "belief updates served by the rank-k covariance update (csrc/k_inc.hip) / by the full solve since the "
                              "engine was created (warm-up script included); the timed update is #37 of the iSAM2 counter: "
                              "incremental (the full solve runs on the 10th updates that relinearise - update_cycle below)"},
    })
    if train is not None:
        out["train_allreduce"] = train
    # the secondary sections and the CPU baselines belong to the N = 1 line only (driver contract)
    if not args.no_policy and world == 1:
        out["policy_path"] = policy_bench(eng, dev)
        out["config5_scale"] = config5_bench(local_rank)
        out["full_fill"] = full_fill_bench(local_rank)
        out["update_cycle"] = update_cycle_bench(local_rank)
        # what a trajectory pays on average (nine rank-k updates and the relinearising tenth, no restore in the timed region):
        # reported beside the headline, whose timed update is always a non-relinearising one
        out["value_trajectory_average"] = {"value": out["update_cycle"]["env_steps_per_sec"], "unit": "env-steps/sec",
                                           "what": "update_cycle: ten consecutive belief updates (37 -> 46 poses) incl. the 10th, relinearising one"}
        out["capacity_256"] = capacity_bench(local_rank)
        out["capacity_256"]["vs_headline"] = out["capacity_256"]["env_steps_per_sec"] / (out["value"] / world)
        out["dqn_loop"] = dqn_loop_bench(local_rank)
        out["a2c_loop"] = a2c_loop_bench(local_rank)
    if not args.no_cpu_baseline and world == 1:
        out["cpu_baseline"] = cpu_baseline()
        out["gpu_over_cpu_thread"] = (out["value"] / world) / out["cpu_baseline"]["value"]
        out["cpu_baseline_all_cores"] = cpu_baseline_all_cores()


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--cpu-worker":  # child of cpu_baseline_all_cores
        n, t = _cpu_worker((int(sys.argv[2]), float(sys.argv[3])))
        print(n, t)
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="after the headline steps, also measure everything else: per-kernel event passes and rooflines, the SLAM "
                         "path split, the DQN-update / gradient all-reduce section, the decision-path / loop / scale sections and "
                         "the CPU baselines (a plain run times the headline steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rank 0's envs) to DIR/<name>.npy, float64")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-policy", action="store_true", help="with --full: skip the secondary decision-path / GCN measurements")
    ap.add_argument("--no-train", action="store_true", help="with --full: skip the DQN-update / gradient all-reduce section")
    ap.add_argument("--print-launch", action="store_true", help="print the multi-rank launch command and exit")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.print_launch):
        # no launcher around us: become one (one rank per GPU, the command the driver uses for N > 1)
        cmd = spawn_command([a for a in sys.argv[1:] if a != "--print-launch"], args.gpus)
        if args.print_launch:
            print(" ".join(cmd))
            return
        import subprocess
        sys.exit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # DRLGX_BENCH_BACKEND=gloo lets the multi-rank control flow be exercised on a box with fewer GPUs than ranks
    # (ranks then share devices); the measured configuration is one rank per GPU over RCCL ("nccl")
    backend = os.environ.get("DRLGX_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    if dist is not None:
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
    eng, cfg = make_engine(local_rank, seed0=rank * N_ENVS)
    odom = torch.tensor([STEP_ACTION] * N_ENVS, dtype=torch.float64, device=dev)
    counts = [eng.counts(i) for i in range(0, N_ENVS, 16)]
    P = float(np.mean([c["poses"] for c in counts]))
    L = float(np.mean([c["landmarks"] for c in counts]))
    M = float(np.mean([c["factors"] for c in counts]))

    def one_step():
        eng.restore(0)
        eng.step(odom)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    eng.check_status()
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    total_steps = args.steps * N_ENVS * world
    out = None if rank != 0 else {
        "metric": "env-steps/sec (256 parallel envs, ~64-node graphs)", "value": total_steps / elapsed,
        "unit": "env-steps/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "configs[1]: 256 envs/GPU, 40x40 map (V=1600), 100 landmarks, belief update at "
                               "~%.0f-node graphs (P=%.1f poses, L=%.1f landmarks, M=%.0f factors) from a device snapshot"
                               % (P + 1 + L, P + 1, L, M),
                   "envs_per_gpu": N_ENVS, "map_size": MAP, "num_landmarks": NUM_LM, "parallelism": "env-sharded x%d" % world},
        "ranks_in_process_group": (dist.get_world_size() if dist is not None else 1),
        "collective_backend": (dist.get_backend() if dist is not None else "none"),
    }
    if args.dump_outputs and rank == 0:
        dump_outputs(eng, args.dump_outputs)
    if args.full:
        full_measurements(args, eng, dev, dist, world, local_rank, one_step, P, L, M, out)
    if rank == 0:
        print(json.dumps(out))
    eng.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
