"""GPU tests of the decision-side read-out where its loops wrap: the graph export (k_graph.hip) on graphs larger than a
workgroup, on batches wider than the offset scan's one-env-per-thread form and on map sizes that are no multiple of 256 cells, its
no-frontier path, and the read-out kernels of k_misc.hip (k_metrics, k_utility, k_line_plan, k_fetch_pack).  The reference of
every comparison is the oracle (OracleEnv / OracleSim / data_process) or a few lines of float64 numpy; every graph comparison
also goes once through the C ABI with sentinel-filled buffers (graph_checks.raw_graph): nothing is written past what is reported."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from graph_checks import check_graph_slice, graph_to_host, oracle_graph, raw_graph  # noqa: E402

MAP = 40
RESET = [(1, 1, math.pi / 2)] * 4  # ExplorationEnv.reset (exploration_env.py:389-422)
DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3


def generic_starts(n, msize=MAP):
    return np.array([O.start_pose(lo, msize / 2 + 20) for lo in range(n)]) + np.array([0.3183, -0.2718, 0.1234])


def step_all(eng, act, active=None):
    odom = torch.tensor([act] * eng.n_envs, dtype=torch.float64, device=eng.device)
    eng.step(odom, None if active is None else torch.as_tensor(active, dtype=torch.uint8, device=eng.device))


def entropy_f64(prob, count_explored):
    """scripts/test.py:61-74 for any map size: -sum p ln p + 0.5 ln 0.5 (V - cells of the unpadded box)."""
    p = np.asarray(prob, dtype=np.float64).reshape(-1)
    return float(-(p * np.log(p)).sum() + 0.5 * np.log(0.5) * (p.size - count_explored))


def check_readout(eng, envs, ids=None):
    """utility / explored / uncertainty_EM / metrics of the engine's envs `ids` against their OracleEnv, with the tolerances of
    test_reset_and_scripted_steps_match_oracle and test_device_metrics_equal_the_host_getters."""
    ids = range(len(envs)) if ids is None else ids
    dist = torch.full((eng.n_envs,), 1.7, dtype=torch.float64, device=eng.device)
    u, ud, ex = eng.utility().cpu().numpy(), eng.utility(dist).cpu().numpy(), eng.explored().cpu().numpy()
    aopt, dopt = eng.uncertainty_em(0).cpu().numpy(), eng.uncertainty_em(1).cpu().numpy()
    m = eng.metrics().cpu().numpy()
    ext_cells = int(2 * 20 // eng.cfg.resolution)
    count_explored = (eng.rows - ext_cells) * (eng.cols - ext_cells)
    for i, env in zip(ids, envs):
        sim = env._sim
        assert u[i] == pytest.approx(sim.calculate_utility(0.0), rel=1e-9)
        assert ud[i] == pytest.approx(sim.calculate_utility(1.7), rel=1e-9)
        assert ex[i] == env.status()
        assert aopt[i] == pytest.approx(sim.uncertainty_em(0), rel=1e-9)
        assert dopt[i] == pytest.approx(sim.uncertainty_em(1), rel=1e-7)
        orc = [env.get_landmark_error(), entropy_f64(sim.virtual_map()[0], count_explored), env.max_uncertainty_of_trajectory()]
        print("env %d metrics %s oracle %s" % (i, m[i], orc))
        np.testing.assert_allclose(m[i][[0, 2]], np.array(orc)[[0, 2]], rtol=1e-8)
        assert m[i][1] == pytest.approx(orc[1], rel=5e-3)
        # ... and the entropy against the same float64 sum over the engine's own exported map (the host-getter comparison)
        np.testing.assert_allclose(m[i][1], entropy_f64(eng.virtual_map(i)[0], count_explored), rtol=1e-12)


# ---- 1. graphs larger than a workgroup --------------------------------------------------------------------------------------

def test_graphs_beyond_256_nodes_and_256_landmarks_match_oracle():
    """BASELINE config 5's world (50 m, 500 landmarks) along a lawn-mower sweep: the export, utility, explored fraction and the
    metric trio against the oracle at 230 nodes (every 256-stride loop of k_graph_build / k_graph_emit / k_metrics makes one
    pass), beyond 256 nodes and beyond 256 landmarks (landmark ranking, nearest frontier per landmark, slot_of_node, the row
    scan and the landmark error sum wrap).  Nothing is left out of any comparison: neither oracle env has a knife-edge cell."""
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    msize = 50
    cfg = default_config(msize, num_landmarks=500, max_poses=80, max_landmarks=500, max_factors=3600)
    starts = np.array([[-21.3183, -19.2718, 0.1234], [21.2817, 19.6282, 3.2134]])
    seeds = np.array([0, 2])
    n = len(seeds)
    eng = Engine(cfg, n, 0)
    envs = [O.OracleEnv(msize, int(seeds[i]), num_landmarks=500, start=tuple(starts[i])) for i in range(n)]
    assert [env.env_index for env in envs] == list(seeds)  # (the reset saw a landmark: no other world was drawn)
    eng.reset(np.arange(n), seeds, starts=starts)
    for act in RESET:
        step_all(eng, act)
    lane = [(2, 0, 0)] * 16
    tl = [(0.5, 0, math.pi / 2)] + [(2, 0, 0)] * 4 + [(0.5, 0, math.pi / 2)]
    tr = [(0.5, 0, -math.pi / 2)] + [(2, 0, 0)] * 4 + [(0.5, 0, -math.pi / 2)]
    script = lane + tl + lane + tr + lane + tl + lane
    sizes = {}
    for s, act in enumerate(script[:74]):
        step_all(eng, act)
        for env in envs:
            env.step(act)
        if s not in (40, 50, 68, 73):
            continue
        assert eng.status() == 0
        for env in envs:
            assert not env._sim.knife_edge_cells(1e-9).any()
        ogs = [oracle_graph(env) for env in envs]
        h = graph_to_host(eng.graph())
        for i in range(n):
            check_graph_slice(h, i, ogs[i])
        if s in (40, 73):  # below and far beyond a workgroup's width: the same through the C ABI, with sentinels
            hr, st = raw_graph(eng)
            assert st == 0
            for i in range(n):
                check_graph_slice(hr, i, ogs[i])
            for k in hr:  # (same state, same kernels: beside the padding of frontier_xy the buffers hold what Engine.graph returned)
                assert k == "frontier_xy" or np.array_equal(hr[k], h[k]), k
        check_readout(eng, envs)
        sizes[s] = [(env._sim.num_poses(), env._sim.num_landmarks(), og["N"], og["edge_index"].shape[1], og["F"]) for env, og in zip(envs, ogs)]
        print("script index %d: (P, L, N, E, F) per env = %s" % (s, sizes[s]))
    # the sizes this test is about were reached (a changed world must not turn it back into a one-pass test)
    assert all(N < 256 for _, _, N, _, _ in sizes[40])
    assert all(N > 256 for _, _, N, _, _ in sizes[50])
    assert all(L > 256 and N > 256 for _, L, N, _, _ in sizes[68])
    assert sizes[68][0] == (74, 260, 363, 3962, 29)
    assert all(P == 79 for P, _, _, _, _ in sizes[73])
    eng.close()


# ---- 2. batch widths of the offset scan -------------------------------------------------------------------------------------

EXTRA = [(2, 0, 0), (1.3, 0, 0.4), (2, 0, 0), (0.7, 0, -0.9), (2, 0, 0)]  # template k takes the first k of these after its reset


@functools.lru_cache(maxsize=None)
def scan_templates():
    """Six oracle envs of the 40 m default world (seeds 0..5, generic starts), template k stepped k times beyond its reset:
    (seeds after the reset's re-draws, starts, oracle graphs).  Computed once, shared by every batch width, never changed."""
    starts = generic_starts(6)
    envs = [O.OracleEnv(MAP, k, start=tuple(starts[k])) for k in range(6)]
    for k, env in enumerate(envs):
        for act in EXTRA[:k]:
            env.step(act)
        assert not env._sim.knife_edge_cells(1e-9).any()
    ogs = [oracle_graph(env) for env in envs]
    assert len(set((og["N"], og["edge_index"].shape[1]) for og in ogs)) > 3  # the scan sums non-uniform values
    return np.array([env.env_index for env in envs]), starts, ogs


@pytest.mark.parametrize("n_envs", [1, 65, 1025, 2100])
def test_batch_offsets_at_scan_widths_match_oracle(n_envs):
    """k_graph_scan at one env, one past a wave, one past its 1024 threads (chunk = 2: a thread with half a range, 511 with none) and 2100
    (chunk = 3: 700 threads with a range): the offsets are the exclusive sums of the per-env counts and every env's
    slice is the oracle graph of its template (env i: seed, start and step count of template i % 6)."""
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    tseeds, tstarts, ogs = scan_templates()
    tid = np.arange(n_envs) % 6
    eng = Engine(default_config(MAP), n_envs, 0)
    eng.reset(np.arange(n_envs), tseeds[tid], starts=tstarts[tid])
    for act in RESET:
        step_all(eng, act)
    for j, act in enumerate(EXTRA):
        step_all(eng, act, active=(tid > j))
    assert eng.status() == 0
    cnt = eng.counts_dev().cpu().numpy()
    assert np.array_equal(cnt[:, 0], 5 + tid) and np.all(cnt[:, 1] >= 1)
    g = eng.graph()
    h = graph_to_host(g)
    hr, st = raw_graph(eng)
    assert st == 0
    n_nodes = np.array([ogs[k]["N"] for k in tid])
    n_edges = np.array([ogs[k]["edge_index"].shape[1] for k in tid])
    for hh in (h, hr):
        assert np.array_equal(hh["node_off"], np.concatenate([[0], np.cumsum(n_nodes)]))
        assert np.array_equal(hh["edge_off"], np.concatenate([[0], np.cumsum(n_edges)]))
    assert np.array_equal(h["batch"], np.repeat(np.arange(n_envs), n_nodes))
    assert np.array_equal(g["node_off_h"], h["node_off"]) and np.array_equal(g["edge_off_h"], h["edge_off"])
    for i in range(n_envs):
        check_graph_slice(h, i, ogs[tid[i]])
    for k in hr:  # (same state, same kernels: beside the padding of frontier_xy the buffers hold what Engine.graph returned)
        assert k == "frontier_xy" or np.array_equal(hr[k], h[k]), k
    print("n_envs %d: %d nodes, %d edges; per template (N, E) = %s" % (n_envs, h["node_off"][-1], h["edge_off"][-1],
                                                                      [(og["N"], og["edge_index"].shape[1]) for og in ogs]))
    eng.close()


# ---- 3. map geometries ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("msize,cells", [(20, 900), (60, 2500), (100, 4900)])
def test_graph_and_readout_on_other_map_sizes(msize, cells):
    """V = 900 / 2500 / 4900 cells (no multiple of 256; 4 / 10 / 20 cells per thread in the frontier compaction, trailing threads
    beyond V) with the reference's integer start of env_index 3 and three forward steps.  The oracle has no knife-edge cell
    in any of the three (asserted), so nothing is masked."""
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    env = O.OracleEnv(msize, 3)
    eng = Engine(default_config(msize), 1, 0)
    assert eng.rows * eng.cols == cells == env._sim.vm_shape()[0] * env._sim.vm_shape()[1]
    # (ExplorationEnv.reset draws another world - env_index + 50 - until the reset sees a landmark: the oracle's final index)
    eng.reset(np.array([0]), np.array([env.env_index]), los=np.array([env.env_index]))
    for act in RESET:
        step_all(eng, act)
    assert eng.counts(0)["landmarks"] == env._sim.num_landmarks() >= 1
    for act in [(2, 0, 0)] * 3:
        step_all(eng, act)
        env.step(act)
        assert not env._sim.knife_edge_cells(1e-9).any()
    assert eng.status() == 0
    og = oracle_graph(env)
    check_graph_slice(graph_to_host(eng.graph()), 0, og)
    hr, st = raw_graph(eng)
    assert st == 0
    check_graph_slice(hr, 0, og)
    check_readout(eng, [env])
    assert np.array_equal(eng.virtual_map(0)[0], env._sim.virtual_map()[0])
    print("map %d: N %d E %d F %d of %d frontier cells, explored %r" % (msize, og["N"], og["edge_index"].shape[1], og["F"],
                                                                      len(env.all_frontiers), env.status()))
    assert og["F"] >= 2 and 0.0 < env.status() < 0.5
    eng.close()


# ---- 4. no frontier, and the one-pose graph ---------------------------------------------------------------------------------

def test_no_frontier_raises_and_exports_the_key_nodes_only():
    """Straight after a reset the virtual map is untouched: no frontier exists, the reference raises (exploration_env.py:327
    indexes an empty list).  The export sets DRLGX_E_INVALID and still writes the L + 1 key nodes and their 2 M edges - the
    P == 1 branches of the pose feature - and nothing else."""
    from drl_graph_exploration_amd import _lib, default_config
    from drl_graph_exploration_amd.engine import Engine
    n = 6
    starts = generic_starts(n)
    ocfg = O.default_config(MAP)
    sims = [O.OracleSim(ocfg, lo, lo, start=tuple(starts[lo])) for lo in range(n)]
    eng = Engine(default_config(MAP), n, 0)  # (its own engine: the status word stays raised)
    eng.reset(np.arange(n), np.arange(n), starts=starts)
    assert eng.status() == 0
    for i in range(n):
        assert np.all(eng.virtual_map(i)[0] == 0.5) and np.all(sims[i].virtual_map()[0] == 0.5)
    h, st = raw_graph(eng)
    assert st == DRLGX_E_INVALID
    seen = set()
    for i, sim in enumerate(sims):
        A, X = sim.adjacency()
        L, M = sim.num_landmarks(), len(sim.factors()[0])
        assert sim.num_poses() == 1 and A.shape[0] == L + 1
        seen.add(min(M, 1))
        # graph_matrix's features (exploration_env.py:236-276) of the key nodes, no frontier node appended
        kp, veh = sim.key_points(), sim.poses()[0][-1]
        feat = np.zeros((L + 1, 5))
        feat[:, 0] = X
        for k in range(L + 1):
            feat[k, 1] = O.OracleEnv.points2dist(kp[k], veh[:2])
            feat[k, 2] = O.OracleEnv.diff_theta(kp[k], veh[:2], veh[2])
        feat[:, 3] = 0.5
        feat[:L, 4], feat[L, 4] = -1, 0
        oei, oea, ox = O.data_process(A, feat)
        assert oei.shape[1] == 2 * M  # 2 (M + P - 1)
        og = dict(N=L + 1, F=0, x=ox, edge_index=oei, edge_attr=oea, frontier_xy=np.zeros((0, 2)), nearest=L + 1)
        check_graph_slice(h, i, og)
    assert seen == {0, 1}, "the templates cover a reset with and one without a measurement"
    assert h["node_off"][n] == sum(s.num_landmarks() + 1 for s in sims) and np.all(h["n_frontier"] == 0)
    assert eng.status() == DRLGX_E_INVALID
    with pytest.raises(_lib.DrlgxError):
        eng.graph()
    eng.close()


# ---- 5. line plans ----------------------------------------------------------------------------------------------------------

def diff_branch(rth, gth):
    """The branch of the ladder in k_line_plan / EMPlanner2D::line_planner (Planner2D.cpp:937-1041) and the margin to its edges."""
    two_pi = 2 * math.pi
    rth, gth = (rth + two_pi if rth < 0 else rth), (gth + two_pi if gth < 0 else gth)
    diff = gth - rth
    branch = 0 if diff > math.pi else 1 if -math.pi < diff < 0 else 2 if diff <= -math.pi else 3
    return branch, min(abs(diff), abs(diff - math.pi), abs(diff + math.pi))


def test_line_plans_in_every_branch_match_oracle():
    """Eight envs turned to headings in all four quadrants, goals on 16 bearings x 5 distances around each (below, just below and
    just above one max_edge_length, several of them, and beyond the map): count exact, actions to 1e-9, and all four branches of
    the bearing ladder taken.  Then the zero-distance goal (each side's own estimated position)."""
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    n = 8
    starts = generic_starts(n)
    ocfg = O.default_config(MAP)
    sims = [O.OracleSim(ocfg, lo, lo, start=tuple(starts[lo])) for lo in range(n)]
    eng = Engine(default_config(MAP), n, 0)
    eng.reset(np.arange(n), np.arange(n), starts=starts)
    # one pure rotation per env towards heading (i + 0.5) pi / 4
    rots = [(0.0, 0.0, O.wrap_theta((i + 0.5) * math.pi / 4 - starts[i][2])) for i in range(n)]
    eng.step(torch.tensor(rots, dtype=torch.float64, device=eng.device))
    for sim, r in zip(sims, rots):
        sim.simulate(r)
    assert eng.status() == 0
    poses = [sim.poses()[0][-1] for sim in sims]
    assert {int((p[2] % (2 * math.pi)) // (math.pi / 2)) for p in poses} == {0, 1, 2, 3}
    dists = (0.37, 1.999, 2.001, 7.3, 37.3)
    cand, goals = [], []
    for i, p in enumerate(poses):
        for k in range(16):
            b = (k + 0.31) * 2 * math.pi / 16
            for d in dists:
                cand.append(i)
                goals.append((p[0] + d * math.cos(b), p[1] + d * math.sin(b)))
    branches = set()
    for c, g in zip(cand, goals):
        p = poses[c]
        br, margin = diff_branch(p[2], math.atan2(g[1] - p[1], g[0] - p[0]))
        d = math.hypot(g[0] - p[0], g[1] - p[1]) / ocfg.max_edge_length
        # (the two sides' poses differ by up to 1e-9: a floor that flips within that of an edge is no finding)
        assert margin > 1e-6 and abs(d - round(d)) > 1e-6
        branches.add(br)
    assert branches == {0, 1, 2, 3}
    actions, n_act = eng.line_plan(torch.tensor(cand, dtype=torch.int32, device=eng.device),
                                   torch.tensor(goals, dtype=torch.float64, device=eng.device))
    acts_h, n_h = actions.cpu().numpy(), n_act.cpu().numpy()
    assert eng.status() == 0
    for c, g in enumerate(goals):
        oa = sims[cand[c]].line_plan(g)
        assert n_h[c] == len(oa)
        np.testing.assert_allclose(acts_h[c, :len(oa)], oa, atol=1e-9)
        assert np.all(acts_h[c, len(oa):] == 0.0)  # (Engine.line_plan hands in zeros: untouched)
    # zero distance: two actions - the turn towards bearing atan2(0, 0) = 0 and an empty translation
    own = [eng.poses(i)[0][-1, :2] for i in range(n)]
    actions, n_act = eng.line_plan(torch.arange(n, dtype=torch.int32, device=eng.device),
                                   torch.tensor(np.array(own), dtype=torch.float64, device=eng.device))
    acts_h, n_h = actions.cpu().numpy(), n_act.cpu().numpy()
    for i in range(n):
        oa = sims[i].line_plan(tuple(poses[i][:2]))
        assert len(oa) == 2 and n_h[i] == 2 and np.all(oa[1] == 0.0) and oa[0][2] != 0.0
        np.testing.assert_allclose(acts_h[i, :2], oa, atol=1e-9)
    assert eng.status() == 0
    eng.close()


def overflow_a_line_plan(eng, sims, starts):
    """Two candidates into sentinel-filled rows of a max_actions = 4 engine: a plan of 20 actions and one of two.  Returns the
    status word after asserting what the rows hold."""
    SENT = -4321.0
    goals = np.array([[starts[0][0] + 37.3 * math.cos(1.0), starts[0][1] + 37.3 * math.sin(1.0)],
                      [starts[1][0] + 0.37 * math.cos(2.0), starts[1][1] + 0.37 * math.sin(2.0)]])
    A = eng.cfg.max_actions
    assert A == 4
    actions = torch.full((3, A, 3), SENT, dtype=torch.float64, device=eng.device)  # (row 2: a guard behind the last candidate)
    n_act = torch.full((3,), -9, dtype=torch.int32, device=eng.device)
    ce = torch.tensor([0, 1], dtype=torch.int32, device=eng.device)
    gd = torch.tensor(goals, dtype=torch.float64, device=eng.device)
    eng.use_torch_stream()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert eng.L.drlgx_line_plan(eng.h, 2, p(ce), p(gd), p(actions), p(n_act)) == 0
    status = eng.status()
    acts_h, n_h = actions.cpu().numpy(), n_act.cpu().numpy()
    o0, o1 = sims[0].line_plan(goals[0]), sims[1].line_plan(goals[1])
    assert len(o0) > A and n_h[0] == len(o0)       # the length the plan needs is reported ...
    np.testing.assert_allclose(acts_h[0], o0[:A], atol=1e-9)  # ... its first four actions are there ...
    assert n_h[1] == len(o1) == 2                  # ... and the neighbouring row is intact
    np.testing.assert_allclose(acts_h[1, :2], o1, atol=1e-9)
    assert np.all(acts_h[1, 2:] == SENT) and np.all(acts_h[2] == SENT) and n_h[2] == -9
    return status


def small_plan_engine():
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    starts = generic_starts(2)
    ocfg = O.default_config(MAP)
    sims = [O.OracleSim(ocfg, lo, lo, start=tuple(starts[lo])) for lo in range(2)]
    eng = Engine(default_config(MAP, max_actions=4), 2, 0)
    eng.reset(np.arange(2), np.arange(2), starts=starts)
    assert eng.status() == 0
    return eng, sims, starts


def test_line_plan_beyond_max_actions_sets_the_status_word_and_keeps_its_row():
    eng, sims, starts = small_plan_engine()
    assert overflow_a_line_plan(eng, sims, starts) == DRLGX_E_CAPACITY
    assert eng.status() == DRLGX_E_CAPACITY
    eng.close()


# ---- 6. status fetch --------------------------------------------------------------------------------------------------------

def test_status_fetch_payload_sizes_and_a_raised_status_word():
    """k_fetch_pack's byte path (sizes that are no multiple of 16, a 16-byte-multiple view 4 bytes into its storage), more than
    one pass of its 256 x 256 threads on either path, and the payload of a read that reports a raised status word."""
    from drl_graph_exploration_amd import _lib
    eng, sims, starts = small_plan_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda k: torch.randint(0, 256, (k,), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)  # noqa: E731
    payloads = [rnd(k) for k in (1, 15, 16, 17, 2 ** 20 + 3, 2 ** 21)]
    base = rnd(4 + 32)
    view = base[4:36]
    assert view.data_ptr() % 16 == 4 and view.numel() % 16 == 0 and payloads[2].data_ptr() % 16 == 0
    payloads.append(view)
    want = [t.cpu().numpy() for t in payloads]
    for t, w in zip(payloads, want):
        got = eng.fetch(t)[0]
        assert got.dtype == np.uint8 and got.shape == w.shape and np.array_equal(got, w)
    assert overflow_a_line_plan(eng, sims, starts) == DRLGX_E_CAPACITY  # (a status, not a fault)
    for t, w in zip(payloads, want):
        host = np.full(w.size + 16, 0xA5, dtype=np.uint8)
        rc = eng.L.drlgx_status_fetch_host(eng.h, C.c_void_p(t.data_ptr()), w.size, host.ctypes.data_as(C.c_void_p))
        assert rc == DRLGX_E_CAPACITY
        assert np.array_equal(host[:w.size], w) and np.all(host[w.size:] == 0xA5)
    with pytest.raises(_lib.DrlgxError):
        eng.fetch(payloads[3])
    assert eng.status() == DRLGX_E_CAPACITY
    eng.close()
