"""GPU tests (run with -m gpu on an MI355X) of the leaf evaluation with non-core steps - the core mask of k_fm2_update /
k_fm2_check (csrc/k_fm2.hip), the mask and the tree distance of k_em_cost (csrc/k_em.hip), k_em_leaves_dubins for every leaf
(csrc/k_em_tree.hip) - and of drlgx_em_plan under the Dubins control model behind Engine.set_dubins_leaf_scoring, against
tests/em_dubins_leaf_ref.py on the cases of tests/em_dubins_leaf_cases.py.  The preconditions of the cases are asserted again on
the engine's own beliefs.

Tolerances: covariances at the project's rtol 1e-6 / atol 1e-10 (tests/test_gpu_fm2.py), reported per band of the masked
measurement count (fm2_cases.band_of); cells' information and A-opt values rel 1e-6, D-opt values rel 8.9e-9 (tests/test_gpu_em.py);
tree poses, per-step rows and leaf distances 1e-9 absolute.  Exact: everything that is a decision or a copy."""
from configparser import ConfigParser

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import em_cases  # noqa: E402
import em_dubins_cases as DC  # noqa: E402
import em_dubins_leaf_cases as LC  # noqa: E402
import em_dubins_leaf_ref as LR  # noqa: E402
import em_dubins_ref as D  # noqa: E402
import em_ref  # noqa: E402
import em_tree_cases as K  # noqa: E402
import em_tree_ref as R  # noqa: E402
import fm2_cases as F  # noqa: E402

ATOL = 1e-9
INFO_RTOL = AOPT_RTOL = 1e-6
DOPT_RTOL = 8.9e-9
DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3


def error_code(call):
    from drl_graph_exploration_amd._lib import DrlgxError
    with pytest.raises(DrlgxError) as ei:
        call()
    return int(str(ei.value).split("drlgx error ")[1].split(":")[0])


def live_state(eng, n):
    out = []
    for i in range(n):
        out += [eng.poses(i)[0], eng.poses(i)[1], eng.landmarks(i)[1], *eng.virtual_map(i)[:3]]
    return [np.array(a, copy=True) for a in out] + [eng.counts_dev().cpu().numpy()]


# ================================================================ the kernels: masks and distances the caller supplies
class Steps(object):
    def __init__(self):
        self.world = LC.steps_world()
        self.eng, self.cfg = F.make_engine(self.world)
        self.dev = self.eng.device
        self._ref, self._cost = {}, {}

    def put(self, cases):
        env, acts, n, core = LC.layout(cases)
        t = lambda a: torch.tensor(a, device=self.dev)  # noqa: E731
        return t(env), t(acts), t(n), t(core)

    def ref(self, name):
        if name not in self._ref:
            e, plan, core = LC.STEP_CASES[name]
            self._ref[name] = LR.fm2_update(self.world.sims[e], plan, core)
        return self._ref[name]

    def cost_ref(self, name, distance=None):
        key = (name, distance)
        if key not in self._cost:
            e, plan, core = LC.STEP_CASES[name]
            sim, cov = self.world.sims[e], self.ref(name)[0]
            u0, c0, info, upd = LR.em_cost(sim, plan, core, distance, 0, cov)
            u1, c1, _, _ = LR.em_cost(sim, plan, core, distance, 1, cov)
            self._cost[key] = (u0, c0, u1, c1, info, upd)
        return self._cost[key]


@pytest.fixture(scope="module")
def steps():
    s = Steps()
    yield s
    s.eng.close()


def test_all_ones_and_no_distance_change_no_bit():
    """Group 1, on the plans of em_cases.plans_for: core = all ones gives the bits of the call without a mask."""
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    n = 4
    sims, starts = em_cases.make_sims(n)
    cfg = default_config(F.MAP, num_landmarks=em_cases.NUM_LANDMARKS, **F.EM_CAPS)
    eng = Engine(cfg, n, 0)
    try:
        eng.reset(np.arange(n), np.arange(n), starts=starts)
        for act in em_cases.SCRIPT:
            eng.step(torch.tensor([act] * n, dtype=torch.float64, device=eng.device))
        cases = [(e, p, [1] * len(p)) for e in range(n) for p in em_cases.plans_for(sims[e], cfg.max_actions)]
        env, acts, na, _ = LC.layout(cases, cfg.max_actions)
        t = lambda a: torch.tensor(a, device=eng.device)  # noqa: E731
        env, acts, na = t(env), t(acts), t(na)
        ones = torch.ones(len(cases), cfg.max_actions, dtype=torch.uint8, device=eng.device)
        cov0, n0 = eng.fm2_update(env, acts, na)
        cov1, n1 = eng.fm2_update(env, acts, na, core=ones)
        assert torch.equal(n0, n1) and cov0.cpu().numpy().tobytes() == cov1.cpu().numpy().tobytes()
        for alg in (0, 1):
            a = eng.em_cost(env, acts, na, alg, want_info=True)
            b = eng.em_cost(env, acts, na, alg, want_info=True, core=ones)
            for x, y in zip(a, b):
                assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert eng.status() == 0 and len(cases) >= 8
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(LC.STEP_CASES))
def test_masked_covariances(steps, name):
    """Groups 2 and 3: all P + K blocks against the masked restatement; the case's own preconditions first."""
    e, plan, core = LC.STEP_CASES[name]
    sim = steps.world.sims[e]
    masked, total, margin = LR.masked_counts(sim, plan, core)
    assert masked == LC.NM[name] and margin > 1e-6, name
    env, acts, na, cm = steps.put([LC.STEP_CASES[name]])
    cov, n_out = steps.eng.fm2_update(env, acts, na, core=cm)
    assert steps.eng.status() == 0
    want, _ = steps.ref(name)
    P, Kn = sim.num_poses(), len(plan)
    assert int(n_out[0]) == P + Kn
    got = cov[0, :P + Kn].cpu().numpy()
    gap = np.abs(got - want) / (F.SIGMA_RTOL * np.abs(want) + F.SIGMA_ATOL)
    print("%s: masked nm %d (band %s), unmasked %d, Sigma' gap / tolerance %.3e" % (name, masked, F.band_of(masked), total, gap.max()))
    np.testing.assert_allclose(got, want, rtol=F.SIGMA_RTOL, atol=F.SIGMA_ATOL, err_msg=name)
    if total > masked:  # the mask is what was compared: the unmasked restatement is far away
        from oracle import fm2_ref
        if total <= F.MAX_MEAS:
            plain, _ = fm2_ref.fm2_update(sim, plan)
            assert (np.abs(plain - want) / (F.SIGMA_RTOL * np.abs(want) + F.SIGMA_ATOL)).max() > 1e3, name


@pytest.mark.parametrize("name", LC.COST_CASES)
def test_masked_costs(steps, name):
    e, plan, core = LC.STEP_CASES[name]
    env, acts, na, cm = steps.put([LC.STEP_CASES[name]])
    u0, c0, info = steps.eng.em_cost(env, acts, na, 0, want_info=True, core=cm)
    u1, c1 = steps.eng.em_cost(env, acts, na, 1, core=cm)
    assert steps.eng.status() == 0
    ru0, rc0, ru1, rc1, rinfo, upd = steps.cost_ref(name)
    info = info[0].reshape(-1, 3).cpu().numpy()
    print("%s: A-opt %.3e D-opt %.3e info %.3e" % (name, abs(float(u0[0]) / ru0 - 1), abs(float(u1[0]) / ru1 - 1),
                                                   (np.abs(info - rinfo) / np.maximum(np.abs(rinfo), 1e-9)).max()))
    np.testing.assert_allclose(info, rinfo, rtol=INFO_RTOL, atol=1e-9, err_msg=name)
    assert float(u0[0]) == pytest.approx(ru0, rel=AOPT_RTOL) and float(c0[0]) == pytest.approx(rc0, rel=AOPT_RTOL), name
    assert float(u1[0]) == pytest.approx(ru1, rel=DOPT_RTOL) and float(c1[0]) == pytest.approx(rc1, rel=DOPT_RTOL), name
    # cells no pose of the leaf's map reaches stay at I / sigma0^2 - those only a non-core step reaches among them
    i0 = 1.0 / steps.world.sims[e].cfg.sigma0 ** 2
    assert np.all(info[~upd] == np.array([i0, 0.0, i0])), name
    if name == "blind_core":
        _, _, _, upd_all = LR.em_cost(steps.world.sims[e], plan, [1] * len(plan))
        only = upd_all & ~upd
        assert only.sum() >= 1 and np.all(info[only] == np.array([i0, 0.0, i0]))
        plain = steps.eng.em_cost(env, acts, na, 0)[0]
        assert abs(float(plain[0]) - float(u0[0])) > 1e-3 * abs(float(u0[0]))


def test_distance_replaces_the_plans_own(steps):
    e, plan, core = LC.STEP_CASES["two_edges"]
    env, acts, na, cm = steps.put([LC.STEP_CASES["two_edges"]])
    d = torch.tensor([LC.TREE_DISTANCE], dtype=torch.float64, device=steps.dev)
    sim = steps.world.sims[e]
    for alg in (0, 1):
        u_a, c_a = steps.eng.em_cost(env, acts, na, alg, core=cm)
        u_b, c_b = steps.eng.em_cost(env, acts, na, alg, core=cm, distance=d)
        u_c, c_c = steps.eng.em_cost(env, acts, na, alg, distance=d)  # (no mask, the distance alone)
        u_p, c_p = steps.eng.em_cost(env, acts, na, alg)
        assert float(u_a[0]) == float(u_b[0]) and float(u_c[0]) == float(u_p[0])
        dw = LR.distance_weight(sim)
        own = em_ref.plan_distance(plan, sim.cfg.angle_weight)
        for with_d, without, u in ((c_b, c_a, u_b), (c_c, c_p, u_c)):
            assert float(with_d[0]) == float(u[0]) + LC.TREE_DISTANCE * dw          # recomputed in float64: the kernel's own sum
            assert float(with_d[0]) - float(without[0]) == pytest.approx((LC.TREE_DISTANCE - own) * dw, rel=1e-12)
    assert steps.eng.status() == 0


def test_the_capacity_counts_core_poses_only(steps):
    """K_max: 1024 unmasked, 128 masked predicted measurements - served (test_masked_covariances); unmasked it is refused, and so
    is its twin of 288 masked ones: DRLGX_E_CAPACITY, live state and the status word untouched."""
    before = live_state(steps.eng, len(steps.world.sims))
    env, acts, na, cm = steps.put([LC.STEP_CASES["K_max"]])
    assert error_code(lambda: steps.eng.em_cost(env, acts, na, 0)) == DRLGX_E_CAPACITY
    steps.eng.em_cost(env, acts, na, 0, core=cm)
    env, acts, na, cm = steps.put([LC.OVER])
    assert LR.masked_counts(steps.world.sims[LC.OVER[0]], LC.OVER[1], LC.OVER[2])[0] > F.MAX_MEAS
    assert error_code(lambda: steps.eng.em_cost(env, acts, na, 0, core=cm)) == DRLGX_E_CAPACITY
    assert steps.eng.status() == 0
    for x, y in zip(before, live_state(steps.eng, len(steps.world.sims))):
        assert x.tobytes() == y.tobytes()


def test_more_candidates_than_one_chunk(steps):
    """130 candidates (chunks of 128): every candidate gets its own mask and distance, whichever chunk it falls into."""
    names = ["K1", "one_edge", "two_edges", "blind_core", "trailing", "fresh_edge"]
    order = [names[i % len(names)] for i in range(130)]
    env, acts, na, cm = steps.put([LC.STEP_CASES[n] for n in order])
    dist = torch.arange(130, dtype=torch.float64, device=steps.dev) * 0.25
    cov, _ = steps.eng.fm2_update(env, acts, na, core=cm)
    unc, cost = steps.eng.em_cost(env, acts, na, 0, core=cm, distance=dist)
    assert steps.eng.status() == 0
    cov, unc, cost = cov.cpu().numpy(), unc.cpu().numpy(), cost.cpu().numpy()
    for i, n in enumerate(order):
        first = order.index(n)
        assert cov[i].tobytes() == cov[first].tobytes() and unc[i] == unc[first], (i, n)
        e = LC.STEP_CASES[n][0]
        assert cost[i] == unc[i] + 0.25 * i * LR.distance_weight(steps.world.sims[e]), (i, n)
    for i in (128, 129):  # the second chunk against the restatement
        want, _ = steps.ref(order[i])
        np.testing.assert_allclose(cov[i][:len(want)], want, rtol=F.SIGMA_RTOL, atol=F.SIGMA_ATOL)


# ================================================================ drlgx_em_plan under the Dubins control model
class Trees(object):
    def __init__(self, max_actions=DC.MAX_ACTIONS):
        from drl_graph_exploration_amd import default_config
        from drl_graph_exploration_amd.engine import Engine
        self.n = DC.N_ENVS
        self.sims = DC.make_sims()
        self.cfg = default_config(K.MAP, num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES, max_actions=max_actions)
        self.eng = Engine(self.cfg, self.n, 0)
        self.eng.reset(np.arange(self.n), np.array(DC.SEEDS), starts=np.array(DC.STARTS))
        for act in K.SCRIPT:
            self.eng.step(torch.tensor([act] * self.n, dtype=torch.float64, device=self.eng.device))
        assert self.eng.status() == 0
        self.dev = self.eng.device
        self.root = [self.eng.poses(i)[0][-1] for i in range(self.n)]
        self.lm = [self.eng.landmarks(i)[:2] for i in range(self.n)]
        self.prob = [self.eng.virtual_map(i)[0].reshape(-1) for i in range(self.n)]

    def i32(self, v):
        return torch.tensor(v, dtype=torch.int32, device=self.dev)

    def use(self, params, sd=0.0, max_nodes=LC.TREE_MAX_NODES, scoring=True):
        self.eng.set_dubins_library(params)
        self.eng.set_sampler_obstacles(sd != 0.0)
        self.eng.set_sampler_parameter(max_nodes, safe_distance=sd, dubins_control_model_enabled=True)
        self.eng.set_dubins_leaf_scoring(scoring)

    def ref(self, name, env, sd, max_nodes=LC.TREE_MAX_NODES):
        keys, xy = self.lm[env]
        return LC.tree_of(self.cfg, self.root[env], self.prob[env], DC.library(name), DC.START_INDICES[env], keys, xy, sd, max_nodes)

    def plan(self, cap=LC.TREE_CAP):
        o = self.eng.em_plan(self.i32(list(range(self.n))), self.i32(DC.START_INDICES), cap, 0, want_nodes=True)
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


@pytest.fixture(scope="module")
def trees():
    t = Trees()
    yield t
    t.eng.close()


def angle_gap(a, b):
    return np.abs(np.arctan2(np.sin(a - b), np.cos(a - b)))


@pytest.mark.parametrize("name, sd", LC.TREE_CASES)
def test_em_plan_under_dubins(trees, name, sd):
    trees.use(DC.LIBS[name], sd)
    try:
        before = live_state(trees.eng, trees.n)
        o = trees.plan()
        assert trees.eng.status() == 0
        lv = {k: (v.cpu().numpy() if v is not None else None) for k, v in trees.eng.em_plan_leaves().items()}
        # the pick is the body of em_cost(core, distance) on the leaves read back, bit for bit
        t = lambda a: torch.tensor(a, device=trees.dev)  # noqa: E731
        again = trees.eng.em_cost(t(lv["cand_env"]), t(lv["actions"]), t(lv["n_actions"]), 0, core=t(lv["core"]), distance=t(lv["distance"]))
        assert again[1].cpu().numpy().tobytes() == lv["cost"].tobytes()
        off, results = 0, []
        for env in range(trees.n):
            ref = trees.ref(name, env, sd)
            tag = "library %s sd %s env %d" % (name, sd, env)
            assert DC.entitled(ref) and not ref.full, tag
            n_nodes = int(o["n_nodes"][env])
            assert n_nodes == len(ref), tag
            nd = o["nodes"][env][:n_nodes]
            np.testing.assert_array_equal(nd[:, 3].astype(np.int64), np.array(ref.parent), err_msg=tag)
            np.testing.assert_array_equal(nd[:, 5:8], np.array(ref.action), err_msg=tag)   # library index, num_steps, 0
            xyt = ref.xytheta()
            dev = max(np.abs(nd[:, :2] - xyt[:, :2]).max(), angle_gap(nd[:, 2], xyt[:, 2]).max(), np.abs(nd[:, 4] - np.array(ref.distance)).max())
            assert dev <= ATOL, (tag, dev)
            assert int(o["result"][env]) == ref.result and int(o["halton_next"][env]) == ref.halton_next, tag
            results.append(ref.result)
            cands = LR.leaf_candidates(ref, trees.cfg.max_actions)
            assert int(o["n_leaves"][env]) == len(cands), tag
            costs = []
            for k, (node, rows, core, dist) in enumerate(cands):
                c = off + k
                assert int(lv["cand_env"][c]) == env and int(lv["n_actions"][c]) == len(rows) == ref.depth[node], tag
                got = lv["actions"][c]
                if len(rows):
                    assert max(np.abs(got[:len(rows), :2] - rows[:, :2]).max(), angle_gap(got[:len(rows), 2], rows[:, 2]).max()) <= ATOL, tag
                assert np.all(got[len(rows):] == 0.0), tag
                np.testing.assert_array_equal(lv["core"][c], core, err_msg=tag)
                assert abs(lv["distance"][c] - dist) <= ATOL, tag
                assert lv["distance"][c] == nd[node, 4], tag   # the tree's own sum (nodes column 4), bit for bit
                masked, _, margin = LR.masked_counts(trees.sims[env], [tuple(r) for r in rows], core)
                assert masked <= F.MAX_MEAS and margin > 1e-9, tag
                costs.append(lv["cost"][c])
            if cands:
                best = R.pick(costs)
                assert int(o["n_actions"][env]) == int(lv["n_actions"][off + best]), tag
                assert o["plan"][env].tobytes() == lv["actions"][off + best].tobytes() and o["cost"][env] == costs[best], tag
                # the winning cost against the numpy restatement (on the oracle's belief of the same seed and script)
                node, rows, core, dist = cands[best]
                _, want, _, _ = LR.em_cost(trees.sims[env], [tuple(r) for r in rows], core, dist)
                print("%s: %d nodes, %d leaves, best %d (%d steps), cost %.6f, restatement %.3e off" % (
                    tag, n_nodes, len(cands), best, len(rows), costs[best], abs(costs[best] / want - 1)))
                assert costs[best] == pytest.approx(want, rel=AOPT_RTOL), tag
            else:
                assert int(o["n_actions"][env]) == 0 and np.all(o["plan"][env] == 0.0), tag
            off += len(cands)
        assert off == len(lv["cost"]) and results.count(R.SUCCESS) >= 2
        if (name, sd) in (("36", 0.0), ("320", DC.SAFE_DISTANCE)):
            assert R.SAMPLING_FAILURE in results
        for x, y in zip(before, live_state(trees.eng, trees.n)):
            assert x.tobytes() == y.tobytes()
    finally:
        trees.eng.set_sampler_obstacles(False)
        trees.eng.set_dubins_leaf_scoring(False)


def test_a_tree_of_no_accepted_node_scores_its_root(trees):
    trees.use(DC.LIB_36, max_nodes=0.0)
    try:
        o = trees.plan()
        lv = trees.eng.em_plan_leaves()
        assert np.all(o["n_nodes"] == 1) and np.all(o["n_leaves"] == 1) and np.all(o["n_actions"] == 0) and np.all(o["plan"] == 0.0)
        assert np.all(o["result"] == R.SUCCESS) and list(o["halton_next"]) == DC.START_INDICES
        assert int(lv["core"].sum()) == 0 and float(lv["distance"].abs().sum()) == 0.0
        z = torch.zeros(trees.n, trees.cfg.max_actions, 3, dtype=torch.float64, device=trees.dev)
        _, root_cost = trees.eng.em_cost(trees.i32(list(range(trees.n))), z, trees.i32([0] * trees.n), 0)
        assert o["cost"].tobytes() == root_cost.cpu().numpy().tobytes()
    finally:
        trees.eng.set_dubins_leaf_scoring(False)


def test_refusals(trees):
    sel, starts = trees.i32(list(range(trees.n))), trees.i32(DC.START_INDICES)
    before = live_state(trees.eng, trees.n)
    trees.use(DC.LIB_320, scoring=False)
    assert error_code(lambda: trees.eng.em_plan(sel, starts, LC.TREE_CAP)) == DRLGX_E_INVALID      # the opt-in off: as before
    trees.eng.set_dubins_leaf_scoring(True)
    trees.eng.em_plan(sel, starts, LC.TREE_CAP)
    trees.eng.set_dubins_library(None)                                                            # on, without a library
    assert error_code(lambda: trees.eng.em_plan(sel, starts, LC.TREE_CAP)) == DRLGX_E_INVALID
    trees.eng.set_dubins_library(DC.LIB_320)
    trees.eng.set_dubins_leaf_scoring(False)                                                      # switched off again
    assert error_code(lambda: trees.eng.em_plan(sel, starts, LC.TREE_CAP)) == DRLGX_E_INVALID
    trees.eng.set_sampler_parameter(0.1)
    assert trees.eng.status() == 0
    for x, y in zip(before, live_state(trees.eng, trees.n)):
        assert x.tobytes() == y.tobytes()


def test_a_leaf_deeper_than_max_actions_refuses_the_call():
    c = Trees(max_actions=5)
    try:
        ref = c.ref("320", 0, 0.0)
        assert DC.entitled(ref) and ref.result == R.SUCCESS and max(ref.depth) > 5
        c.use(DC.LIB_320)
        before = live_state(c.eng, c.n)
        sel, starts = c.i32(list(range(c.n))), c.i32(DC.START_INDICES)
        assert error_code(lambda: c.eng.em_plan(sel, starts, LC.TREE_CAP)) == DRLGX_E_CAPACITY
        assert c.eng.status() == 0
        for x, y in zip(before, live_state(c.eng, c.n)):
            assert x.tobytes() == y.tobytes()
    finally:
        c.eng.close()


# ================================================================ the facades
def dubins_ini(lo, p):
    cp = ConfigParser()
    cp.read_dict({
        "Sensor Model": dict(bearing_noise="0.5", range_noise="0.02", min_bearing="-179.9", max_bearing="179.9", min_range="0.1", max_range="6.0"),
        "Control Model": dict(translation_noise="0.1", rotation_noise="0.2"),
        "Environment": dict(min_x="-6", max_x="6", min_y="-6", max_y="6", max_steps="5000", safe_distance="0.0"),
        "Virtual Map": dict(resolution="2.0", sigma0="1.0", num_samples="1"),
        "Simulator": dict(seed=str(lo), lo=str(lo), num=str(K.NUM_LANDMARKS), sigma_x0="0.05", sigma_y0="0.05", sigma_theta0="0.01"),
        "Planner": dict(seed=str(K.DEFAULT_SEED), angle_weight="0.4", distance_weight0="5.0", distance_weight1="2.0", d_weight="0.0",
                        max_edge_length="2.0", max_nodes="0.1", occupancy_threshold="0.4", safe_distance="0.0", algorithm="EM_AOPT",
                        reg_out="false", dubins_control_model_enabled="true"),
        "Dubins": dict(zip(D.FIELDS, [repr(x) for x in p.values()])),
    })
    return cp


def test_facades():
    from drl_graph_exploration_amd import planner2d
    from drl_graph_exploration_amd.pyplanner2d import EMExplorer
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    h0 = planner2d.halton_start_index(K.DEFAULT_SEED)
    ex = EMExplorer(dubins_ini(0, DC.LIB_320), start=tuple(DC.STARTS[0]), dubins_paths=True)
    try:
        for act in K.SCRIPT:
            ex.simulate(act)
        with pytest.raises(NotImplementedError):   # without the new flag: as before
            ex.plan()
    finally:
        ex.engine.close()
    ex = EMExplorer(dubins_ini(0, DC.LIB_320), start=tuple(DC.STARTS[0]), dubins_paths=True, dubins_leaf_scoring=True)
    try:
        for act in K.SCRIPT:
            ex.simulate(act)
        assert ex.plan()
        out = ex._planner.last
        na = int(out["n_actions"][0])
        plan = out["plan"][0, :na].cpu().numpy()
        edges = list(ex._planner.iter_solution())   # leaf first
        assert na >= 3 and len(edges) >= 1
        odoms = []
        for edge in edges:
            assert len(edge.get_odoms()) == len(edge.second.poses) == edge.second.key - edge.first.key   # num_steps odometries
            odoms = [[p.x, p.y, p.theta] for p in edge.get_odoms()] + odoms
        np.testing.assert_array_equal(np.array(odoms)[:, :2], plan[:, :2])
        np.testing.assert_allclose(np.array(odoms)[:, 2], plan[:, 2], rtol=0, atol=1e-15)
    finally:
        ex.engine.close()
    from staged_facade import StagedEMExplorer
    ex = StagedEMExplorer(dubins_ini(0, DC.LIB_320), start=tuple(DC.STARTS[0]))
    try:
        for act in K.SCRIPT:
            ex.simulate(act)
        models = (ex._sim.sensor_model, ex._sim.control_model)
        with pytest.raises(NotImplementedError):
            planner2d.EMPlanner2D(ex._planner_params, *models, dubins_paths=True).optimize2(ex._slam, ex._virtual_map)
        planner = planner2d.EMPlanner2D(ex._planner_params, *models, dubins_paths=True, dubins_leaf_scoring=True)
        assert planner.halton_next == h0
        assert planner.optimize2(ex._slam, ex._virtual_map) == planner2d.OptimizationResult.SUCCESS
        edges = list(planner.iter_solution())
        assert len(edges) >= 1 and all(len(e.get_odoms()) == e.second.key - e.first.key >= 3 for e in edges)
    finally:
        ex.engine.close()
    env = VecExplorationEnv(K.MAP, 2, env_index=0, test=True, starts=DC.STARTS[:2], num_landmarks=K.NUM_LANDMARKS, max_poses=K.MAX_POSES,
                            n_rollouts=0)
    try:
        e = env.engine
        sel = torch.arange(2, dtype=torch.int32, device=env.device)
        st = torch.full((2,), h0, dtype=torch.int32, device=env.device)
        par = planner2d.DubinsParameter()
        for f, v in zip(D.FIELDS, DC.LIB_320.values()):
            setattr(par, f, v)
        e.set_dubins_library(par)
        e.set_sampler_parameter(0.1, dubins_control_model_enabled=True)
        e.set_dubins_leaf_scoring(True)
        want = {k: v.cpu().numpy() for k, v in e.em_plan(sel, st, 2048, int(env.cfg.algorithm)).items() if v is not None}
        e.set_dubins_leaf_scoring(False)
        e.set_sampler_parameter(0.1)
        e.set_dubins_library(None)
        acts, n_act, result = env.em_plan(max_nodes=0.1, dubins=par)
        np.testing.assert_array_equal(acts.cpu().numpy(), want["plan"])
        np.testing.assert_array_equal(n_act.cpu().numpy(), want["n_actions"])
        np.testing.assert_array_equal(result.cpu().numpy(), want["result"])
        np.testing.assert_array_equal(env._halton_next.cpu().numpy(), want["halton_next"])
        assert int(want["n_actions"].max()) >= 3
        assert e.sampler_parameter == (0.1, 0.0, False) and e.dubins_leaf_scoring is False and e.sampler_obstacles is False
        lv = e.em_plan_leaves()                  # (the call ran with steps, whatever the flag says now: the distances are there)
        assert lv["distance"] is not None and lv["distance"].numel() == lv["cost"].numel() >= 2
        e.set_sampler_parameter(0.1, dubins_control_model_enabled=True)   # the opt-in is back off: the flag alone is refused again
        assert error_code(lambda: e.em_plan(sel, st, 2048, int(env.cfg.algorithm))) == DRLGX_E_INVALID
        e.set_sampler_parameter(0.1)
        e.em_plan(sel, st, 2048, int(env.cfg.algorithm))                  # a call without steps: no distance is kept
        assert e.em_plan_leaves()["distance"] is None
    finally:
        env.close()
