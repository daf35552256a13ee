"""GPU tests (run with -m gpu on an MI355X) of the kernels that walk the grid - k_map / k_map_c, k_og_cost, k_em_cost, k_graph_build,
k_em_tree, k_cov_array, k_metrics and the move bounds check of k_sim - on the rectangular, off-centre worlds of tests/rect_cases.py
(27 x 23 and 23 x 27 cells, four distinct bounds, ragged last tiles of different widths in the two directions) and at the 8-cell
candidate window, against the CPU oracle and the float64 restatements og_ref / em_ref / em_tree_ref.  tests/test_rect_cpu.py
checks the cases themselves on the CPU (no knife edge: nothing is masked here).

No tolerance of its own: every comparison is made by the helper of the square-map test of the same kernel (compare_state,
check_readout, check_graph_slice, the og / em Ctx checks, check_tree) with that test's tolerances."""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_ref  # noqa: E402
import em_tree_cases as K  # noqa: E402
import em_tree_ref as R  # noqa: E402
import rect_cases as RC  # noqa: E402
import test_gpu_em as TEM  # noqa: E402
import test_gpu_em_tree as TT  # noqa: E402
import test_gpu_og as TOG  # noqa: E402
from graph_checks import check_graph_slice, graph_to_host, oracle_graph, raw_graph  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)
from test_gpu_belief import compare_state  # noqa: E402
from test_gpu_graph_edges import check_readout  # noqa: E402

N = RC.N_ENVS


def make_engine(name, n=N, max_poses=RC.MAX_POSES):
    from drl_graph_exploration_amd.engine import Engine
    eng = Engine(RC.engine_config(name, max_poses), n, 0)
    assert (eng.rows, eng.cols) == RC.SHAPES[name]
    return eng


def step_all(eng, act):
    eng.step(torch.tensor([act] * eng.n_envs, dtype=torch.float64, device=eng.device))


def assert_same_bits(a, b, tag):
    """Two engines stepped alike: state, virtual map and the map stage's sums bit for bit (test_compact_map_kernel_equals_the_resident_one)."""
    for i in range(a.n_envs):
        for x, y in zip(a.poses(i) + a.landmarks(i) + a.virtual_map(i), b.poses(i) + b.landmarks(i) + b.virtual_map(i)):
            np.testing.assert_array_equal(x, y, err_msg=tag)
    np.testing.assert_array_equal(a.utility().cpu().numpy(), b.utility().cpu().numpy(), err_msg=tag)
    np.testing.assert_array_equal(a.uncertainty_em(1).cpu().numpy(), b.uncertainty_em(1).cpu().numpy(), err_msg=tag)
    np.testing.assert_array_equal(a.explored().cpu().numpy(), b.explored().cpu().numpy(), err_msg=tag)


def run_three_ways(name):
    """Reset and the world's script on the fused kernel, on the stage kernels with the resident form of the map kernel and on the
    stage kernels with the compact form asked for: status 0 throughout, the first against the oracle after every step (every cell,
    nothing masked), the other two bit-equal to each other and equal to the oracle."""
    fused, res, com = make_engine(name), make_engine(name), make_engine(name)
    res.timing_enable(2)
    com.timing_enable(2)
    sims = RC.fresh_sims(name)
    for e in (fused, res, com):
        e.reset(np.arange(N), np.arange(N), starts=RC.STARTS[name])
        assert e.status() == 0
    for i in range(N):
        compare_state(fused, i, sims[i], "%s reset env %d" % (name, i), check_vm=False)
    was = fused.L.drlgx_debug_map_form(0)
    try:
        for s, act in enumerate(RC.script_of(name)):
            step_all(fused, act)
            fused.L.drlgx_debug_map_form(0)
            step_all(res, act)
            res.synchronize()
            fused.L.drlgx_debug_map_form(1)
            step_all(com, act)
            com.synchronize()
            fused.L.drlgx_debug_map_form(0)
            for sim in sims:
                assert sim.simulate(act) == 0
            assert [e.status() for e in (fused, res, com)] == [0, 0, 0], "%s step %d" % (name, s)
            assert_same_bits(res, com, "%s step %d: resident against compact" % (name, s))
            for i in range(N):
                compare_state(fused, i, sims[i], "%s fused step %d env %d" % (name, s, i))
                compare_state(com, i, sims[i], "%s staged step %d env %d" % (name, s, i))
    finally:
        fused.L.drlgx_debug_map_form(was)
    tm = res.timing_read()
    assert tm["slam"][1] == len(RC.script_of(name)) and tm["step"][1] == 0  # the staged engines really ran the stage kernels
    return fused, res, com, sims


def close_all(*engines):
    for e in engines:
        e.close()


# ---- 1. belief step -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide", "tall", "sector"])
def test_belief_step_on_a_rectangle_matches_the_oracle_in_every_form(name):
    """27 x 23 / 23 x 27 cells: the trajectories of rect_cases.SCRIPT run into columns >= 23 ("wide") / rows >= 23 ("tall"), their
    windows hang over all four grid edges.  The full-circle worlds are served by the compact form when it is asked for, the +-75
    degree sensor never is (its bounding box prunes: one mask per cell does not do)."""
    fused, res, com, _ = run_three_ways(name)
    assert com.L.drlgx_debug_map_compact_ok(com.h, RC.MAX_POSES) == (0 if name == "sector" else 1)
    close_all(fused, res, com)


def test_two_pose_chunks_on_a_rectangle():
    """P = 64, 65, 67 on "wide": the map kernel's second chunk of poses (one mask bit per pose of a chunk).  mask_knife_edge as the
    long soaks pass it - and the masked share is 0 in this oracle run, so every cell is compared."""
    n = 2
    eng = make_engine("wide", n=n, max_poses=72)
    cfg = RC.oracle_config("wide")
    sims = [O.OracleSim(cfg, i, i, start=tuple(RC.CHUNK_STARTS[i])) for i in range(n)]
    eng.reset(np.arange(n), np.arange(n), starts=RC.CHUNK_STARTS)
    seen = []
    for s in range(RC.CHUNK_STEPS):
        act = RC.CHUNK_LOOP[s % len(RC.CHUNK_LOOP)]
        step_all(eng, act)
        for sim in sims:
            assert sim.simulate(act) == 0
        if s in RC.CHUNK_CHECKS or s == RC.CHUNK_STEPS - 1:
            assert eng.status() == 0
            seen.append(sims[0].num_poses())
            for i in range(n):
                assert int(sims[i].knife_edge_cells().sum()) == 0
                compare_state(eng, i, sims[i], "chunks env %d step %d" % (i, s), mask_knife_edge=True)
    assert seen == [64, 65, 67] and eng.counts(1)["poses"] == 67
    eng.close()


# ---- 2. the move bounds check ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide", "tall"])
def test_bounds_probes_are_accepted_and_rejected_as_the_oracle_does(name):
    """One probe per side of the map box, each a single increment that the predicate with the x and y bounds exchanged would judge
    the other way (tests/test_rect_cpu.py): accepted / rejected as the oracle, pose counts equal, state equal afterwards."""
    probes = RC.PROBES[name]
    n = len(probes)
    eng = make_engine(name, n=n)
    cfg = RC.oracle_config(name)
    starts = np.array([p[0] for p in probes])
    sims = [O.OracleSim(cfg, i, i, start=tuple(starts[i])) for i in range(n)]
    eng.reset(np.arange(n), np.arange(n), starts=starts)
    eng.step(torch.tensor([p[1] for p in probes], dtype=torch.float64, device=eng.device))
    assert eng.status() == 0
    verdicts = []
    for i, (_, odom) in enumerate(probes):
        rejected = sims[i].simulate(odom) == 1
        verdicts.append(rejected)
        assert eng.counts(i)["poses"] == sims[i].num_poses() == (1 if rejected else 2), (name, i)
        compare_state(eng, i, sims[i], "%s probe %d" % (name, i), check_vm=not rejected)
    assert sorted(verdicts) == [False, False, True, True]
    # ... and the next, ordinary step is the oracle's too (a rejected move left nothing behind)
    step_all(eng, (1.3, 0.0, 0.4))
    for i in range(n):
        sims[i].simulate((1.3, 0.0, 0.4))
        compare_state(eng, i, sims[i], "%s step after probe %d" % (name, i))
    assert eng.status() == 0
    eng.close()


# ---- 3. read-outs, graph export, line plans -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide", "tall"])
def test_readouts_graph_and_line_plans_on_a_rectangle(name):
    eng = make_engine(name)
    envs = RC.make_envs(name)  # (their constructor has run the reset's four actions)
    eng.reset(np.arange(N), np.arange(N), starts=RC.STARTS[name])
    for act in RC.RESET:
        step_all(eng, act)
    for act in RC.SCRIPT[4:]:
        step_all(eng, act)
        for env in envs:
            env.step(act)
    assert eng.status() == 0
    for i, env in enumerate(envs):
        assert env.env_index == i and not env._sim.knife_edge_cells(1e-9).any()
        compare_state(eng, i, env._sim, "%s env %d" % (name, i))
    # utility, explored, both EM uncertainties, the metric trio with count_explored = (rows - 20)(cols - 20)
    assert (eng.rows - 20) * (eng.cols - 20) == 21
    check_readout(eng, envs)
    # cov_array against numpy's symmetric eigen-decomposition of every updated cell's covariance (test_gpu_modules)
    ln, an = (t.cpu().numpy() for t in eng.cov_array())
    assert ln.shape == an.shape == (N,) + RC.SHAPES[name]
    for i in range(N):
        _, info, _, upd = eng.virtual_map(i)
        assert upd.sum() > 40
        for idx in np.flatnonzero(upd):
            w, vec = np.linalg.eigh(np.linalg.inv(info[idx]))
            r, c = divmod(int(idx), eng.cols)
            assert ln[i, r, c] == pytest.approx(min(math.sqrt(w[1]), 1.0), rel=1e-9)
            assert abs(math.sin(math.atan2(vec[1, 1], vec[0, 1]) - an[i, r, c])) < 1e-6
        assert np.all(ln[i].reshape(-1)[upd == 0] == 1.0)
    # graph export, once more through the C ABI with sentinels
    ogs = [oracle_graph(env) for env in envs]
    h = graph_to_host(eng.graph())
    hr, st = raw_graph(eng)
    assert st == 0
    for i in range(N):
        check_graph_slice(h, i, ogs[i])
        check_graph_slice(hr, i, ogs[i])
    assert all(og["F"] >= 1 for og in ogs)
    # line plans to every frontier
    cand = [i for i, env in enumerate(envs) for _ in env._frontier]
    goals = [tuple(f) for env in envs for f in env._frontier]
    actions, n_act = eng.line_plan(torch.tensor(cand, dtype=torch.int32, device=eng.device), torch.tensor(goals, dtype=torch.float64, device=eng.device))
    acts_h, n_h = actions.cpu().numpy(), n_act.cpu().numpy()
    assert eng.status() == 0
    for c, (i, g) in enumerate(zip(cand, goals)):
        oa = envs[i]._sim.line_plan(g)
        assert n_h[c] == len(oa) and len(oa) >= 2
        np.testing.assert_allclose(acts_h[c, :len(oa)], oa, atol=1e-9)
    eng.close()


# ---- 4. cost kernels and the tree sampler, from the belief after the script -------------------------------------------------------

class RectCtx(TOG.Ctx):
    """test_gpu_og's Ctx on one world of rect_cases, with the expected look-ahead cost's plans and references beside it."""

    def __init__(self, name):
        TOG.Ctx.__init__(self, name, cases=RC.OgView(name))
        self.og_plans = self.plans
        self.em_plans = [RC.em_plans_for(s) for s in self.sims]
        self._em_ref = {}
        self.A = RC.MAX_ACTIONS

    def em_ref_of(self, e, k):
        if (e, k) not in self._em_ref:
            self._em_ref[(e, k)] = em_ref.em_costs(self.sims[e], self.em_plans[e][k])
        return self._em_ref[(e, k)]


_ctx = {}


@pytest.fixture(scope="module")
def ctx():
    def get(name):
        if name not in _ctx:
            _ctx[name] = RectCtx(name)
        return _ctx[name]
    yield get
    for c in _ctx.values():
        c.eng.close()
    _ctx.clear()


@pytest.mark.parametrize("name", ["wide", "tall", "sector"])
def test_og_cost_on_a_rectangle_matches_the_restatement(ctx, name):
    """K = 0, 1, the spiral of max_actions and a run out of the map box: every cell's bits, the sums at test_gpu_og's SUM_RTOL."""
    c = ctx(name)
    assert c.plans is c.og_plans
    before = c.live_state()
    ce, acts, nact = c.device_candidates(c.cases)
    ent, cost, prob = (t.cpu().numpy() for t in c.eng.og_cost(ce, acts, nact, want_prob=True))
    assert c.eng.status() == 0 and prob.shape[1:] == RC.SHAPES[name]
    for i, case in enumerate(c.cases):
        c.check(case, ent[i], cost[i], prob[i], "%s env %d plan %d" % ((name,) + case))
    for a, b in zip(before, c.live_state()):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["wide", "tall", "sector"])
def test_em_cost_on_a_rectangle_matches_the_restatement(ctx, name):
    """The same plans (the spiral cut to 256 predicted measurements) at test_gpu_em's tolerances, both algorithms."""
    c = ctx(name)
    before = c.live_state()
    c.plans = c.em_plans
    try:
        ce, acts, nact = c.device_candidates(c.cases)
    finally:
        c.plans = c.og_plans
    assert [int(k) for k in nact[2::4]] == [RC.MAX_ACTIONS] * N  # (the spiral at its full length: nothing was cut)
    unc0, cost0, info = c.eng.em_cost(ce, acts, nact, 0, want_info=True)
    unc1, cost1 = c.eng.em_cost(ce, acts, nact, 1)
    assert c.eng.status() == 0
    unc0, cost0, info, unc1, cost1 = (t.cpu().numpy() for t in (unc0, cost0, info, unc1, cost1))
    shim = types.SimpleNamespace(ref=c.em_ref_of, sims=c.sims)
    for i, (e, k) in enumerate(c.cases):
        assert min(c.em_ref_of(e, k)[3].values()) > 1e-9
        TEM._check_against_ref(shim, e, k, unc0[i], cost0[i], unc1[i], cost1[i], info[i], "%s env %d plan %d" % (name, e, k))
    for a, b in zip(before, c.live_state()):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_tree_sampler_on_a_rectangle_matches_the_restatement(ctx, name):
    """em_plan (65 accepted nodes) and rrt_plan (a goal far across the grid) against em_tree_ref.grow with the map's own bounds:
    the samples spread over span_x x span_y from (min_x, min_y), node for node."""
    c = ctx(name)
    eng, cfg = c.eng, c.cfg
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=eng.device)  # noqa: E731
    before = c.live_state()
    for env in range(N):
        root = eng.poses(env)[0][-1]
        known = int(np.count_nonzero(eng.virtual_map(env)[0] < cfg.occupancy_threshold))
        start = K.START_INDICES[env]
        eng.set_sampler_parameter(K.max_nodes_for(known, RC.TREE_NODES))
        o = TT.host(eng.em_plan(i32([env]), i32([start]), K.CAP, 0, want_nodes=True))
        assert eng.status() == 0
        t = K.tree_of(cfg, root, start, n_accept=RC.TREE_NODES)
        assert min(t.margin) > K.MARGIN
        tag = "%s env %d" % (name, env)
        TT.check_tree(o["nodes"][0], int(o["n_nodes"][0]), t, tag)
        assert int(o["result"][0]) == R.SUCCESS and int(o["halton_next"][0]) == t.halton_next
        lv, _ = TT.leaves_of(o["nodes"][0], int(o["n_nodes"][0]))
        assert lv == t.leaves() and int(o["n_leaves"][0]) == len(lv), tag
        goal = RC.RRT_GOALS[name][env]
        o = TT.host(eng.rrt_plan(i32([env]), i32([10 ** 6]), torch.tensor(goal[None, :], device=eng.device), i32([start]), K.CAP, want_nodes=True))
        assert eng.status() == 0
        g = K.tree_of(cfg, root, start, goal=tuple(goal))
        assert min(g.margin) > K.MARGIN and g.result == R.SUCCESS
        TT.check_tree(o["nodes"][0], int(o["n_nodes"][0]), g, "rrt " + tag)
        na = int(o["n_actions"][0])
        assert int(o["result"][0]) == R.SUCCESS and na == g.depth[g.goal_node] and int(o["halton_next"][0]) == g.halton_next
        np.testing.assert_allclose(o["plan"][0, :na], np.array(g.actions_to(g.goal_node)), atol=TT.ATOL)
    for a, b in zip(before, c.live_state()):
        np.testing.assert_array_equal(a, b)


# ---- 5. the 8-cell window -------------------------------------------------------------------------------------------------------

def test_the_8_cell_window_in_every_form():
    """max_range = 7 at resolution 2: an 8-cell window, the limit of the 8 x 8 slot grid, and poses whose disc holds 41 cell centres
    (tests/test_rect_cpu.py) - more than the 40 per pose the compact stage is carved for.  Such an engine is kept on the resident
    form (k_map.hip: map_lds_bytes_compact, by the host's bound on the lattice count) also when the compact one is asked for; before
    that rule the forced compact form raised DRLGX_E_CAPACITY at the first rebuild and left the map alone."""
    fused, res, com, sims = run_three_ways("win8")
    # (envs 0 and 2 stand on 41-cell spots, env 1 on a generic one.  With the rule in place both staged engines run the resident
    # form - asserted below - so their bit-equality says that ASKING for the compact form changes nothing here.)
    assert max(RC.in_range_cells(sims[0])) == max(RC.in_range_cells(sims[2])) == 41 and max(RC.in_range_cells(sims[1])) < 41
    assert com.L.drlgx_debug_map_compact_ok(com.h, RC.MAX_POSES) == 0
    close_all(fused, res, com)


def test_a_9_cell_window_is_refused_at_creation():
    from drl_graph_exploration_amd import _lib
    from drl_graph_exploration_amd.engine import Engine
    cfg = RC.engine_config("win8")
    cfg.max_range = 7.5
    with pytest.raises(_lib.DrlgxError, match="cell window"):
        Engine(cfg, 1, 0)
