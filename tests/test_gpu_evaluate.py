"""GPU tests of the evaluation driver: the device-side greedy pick (drlgx_greedy_plans), the traced plan execution with its
device-side stop at done (drlgx_step_plans_traced) and `evaluate()` over them, against the per-action primitives the driver
replaces and against the reference's pinned result rows."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAP = 40


# ---------------------------------------------------------------------------------------------------------------------
# 1. the pick
# ---------------------------------------------------------------------------------------------------------------------
def _scores(pattern, n, rng):
    s = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    if n == 0:
        return s
    if pattern == "max_first":
        s[0] = 2.0
    elif pattern == "max_last":
        s[n - 1] = 2.0
    elif pattern == "tie_63_64":  # (two equal maxima, in lane 63 and - where the stride wraps - in lane 0's second element)
        s[min(63, n - 1)] = 2.0
        s[min(64, n - 1)] = 2.0
    elif pattern == "all_equal":
        s[:] = 0.5
    elif pattern == "neg_inf_but_one":
        s[:] = -np.inf
        s[n // 2] = -3.0
    elif pattern == "nan_after_larger":
        s[0] = 5.0
        s[n - 1] = np.nan
    elif pattern == "two_nans":
        s[n // 3] = np.nan
        s[n - 1] = np.nan
    return s


def _pick_reference(score, seg_begin, nfr, active, actions_pad, n_act_pad):
    n, _, A, _ = actions_pad.shape
    choice = np.full(n, -1, dtype=np.int32)
    acts = np.zeros((n, A, 3))
    nact = np.zeros(n, dtype=np.int32)
    for e in range(n):
        if not active[e] or nfr[e] == 0:
            continue
        c = int(np.argmax(score[seg_begin[e]:seg_begin[e] + nfr[e]]))
        choice[e] = c
        nact[e] = n_act_pad[e, c]
        acts[e, :nact[e]] = actions_pad[e, c, :nact[e]]
    return choice, acts, nact


@pytest.mark.parametrize("layout", ["dqn", "a2c"])
def test_greedy_pick_equals_numpy_argmax(layout):
    """Segments of 1, 3, 64, 65, 70 and 0 frontiers (64 / 65: where the wave's stride over the segment wraps) under every score
    pattern, an inactive env among them, in the read-out layout of both callers: choice, plan length and every byte of the
    plan must equal the numpy restatement."""
    from drl_graph_exploration_amd.engine import Engine
    rng = np.random.RandomState(5)
    MF, A = 70, 4
    patterns = ["max_first", "max_last", "tie_63_64", "all_equal", "neg_inf_but_one", "nan_after_larger", "two_nans"]
    cases = [(n, p) for n in (1, 3, 64, 65, 70, 0) for p in patterns]
    nfr = np.array([c[0] for c in cases] + [5, 70], dtype=np.int32)
    active = np.ones(len(nfr), dtype=np.uint8)
    active[-2:] = 0  # (the two extra envs have frontiers and scores, and are switched off)
    segs = [_scores(p, n, rng) for n, p in cases] + [_scores("max_last", 5, rng), _scores("max_first", 70, rng)]
    n = len(nfr)
    if layout == "dqn":  # every graph's other nodes come first, with values above every frontier's: reading outside shows
        other = rng.randint(0, 9, size=n)
        score = np.concatenate([np.concatenate([np.full(other[e], 100.0, dtype=np.float32), segs[e]]) for e in range(n)])
        node_off = np.concatenate([[0], np.cumsum(other + nfr)]).astype(np.int32)
        seg_begin = node_off[1:] - nfr
    else:
        score = np.concatenate(segs)
        seg_begin = (np.cumsum(nfr) - nfr).astype(np.int32)
    actions_pad = rng.normal(size=(n, MF, A, 3))
    n_act_pad = rng.randint(0, A + 1, size=(n, MF)).astype(np.int32)
    n_act_pad[:, 0] = A
    n_act_pad[:, 1] = 0
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    choice, acts, nact = Engine.greedy_plans(t(score), t(seg_begin), t(nfr), t(actions_pad), t(n_act_pad), t(active))
    torch.cuda.synchronize()
    want_c, want_a, want_n = _pick_reference(score, seg_begin, nfr, active, actions_pad, n_act_pad)
    np.testing.assert_array_equal(choice.cpu().numpy(), want_c)
    np.testing.assert_array_equal(nact.cpu().numpy(), want_n)
    assert acts.cpu().numpy().tobytes() == want_a.tobytes()
    # the patterns did what their names say (the restatement is numpy's own arg-max: this guards the test's inputs)
    by = {c: want_c[i] for i, c in enumerate(cases)}
    assert by[(70, "max_last")] == 69 and by[(65, "tie_63_64")] == 63 and by[(70, "tie_63_64")] == 63 and by[(65, "all_equal")] == 0
    assert by[(65, "nan_after_larger")] == 64 and by[(70, "two_nans")] == 23 and by[(64, "neg_inf_but_one")] == 32
    assert by[(0, "max_first")] == -1 and want_c[-1] == -1 and want_c[-2] == -1
    # without the mask the two extra envs are picked like the others
    choice2, _, _ = Engine.greedy_plans(t(score), t(seg_begin), t(nfr), t(actions_pad), t(n_act_pad))
    assert choice2.cpu().numpy()[-2:].tolist() == [4, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the traced execution against one call per action
# ---------------------------------------------------------------------------------------------------------------------
def _fresh(n):
    """n envs on the seeds 0 .. n - 1 with every env's plan to its nearest frontier (frontier slot 0)."""
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    env = VecExplorationEnv(MAP, n, env_index=0, test=True, n_rollouts=0)
    g = env.engine.graph(plan=True)
    acts = g["actions_pad"][:, 0].contiguous()
    nact = g["n_act_pad"][:, 0].contiguous()
    assert int(g["n_frontier"].min()) >= 1
    return env, acts, nact


def _state(eng, n):
    out = []
    for i in range(n):
        xyt, info = eng.poses(i)
        prob, vinfo, tr, upd = eng.virtual_map(i)
        out.append([xyt, info, prob, vinfo, tr, upd])
    return eng.counts_dev().cpu().numpy(), out


def _assert_state_equal(a, b, envs):
    np.testing.assert_array_equal(a[0][envs], b[0][envs])
    for i in envs:
        for x, y in zip(a[1][i], b[1][i]):
            assert x.tobytes() == y.tobytes()


@functools.lru_cache(maxsize=None)
def _run_a(n):
    """Engine A: one step_plan + metrics() + explored() per action index.  Returns host arrays, computed once per n."""
    env, acts, nact = _fresh(n)
    eng = env.engine
    counts0 = eng.counts_dev().cpu().numpy()
    nact_h = nact.cpu().numpy()
    A = env.cfg.max_actions
    trace = np.full((n, A, 4), np.nan)
    for k in range(int(nact_h.max())):
        eng.step_plan(acts, nact, k, map_last_only=False)
        m = eng.metrics().cpu().numpy()
        x = eng.explored().cpu().numpy()
        on = nact_h > k
        trace[on, k, :3] = m[on]
        trace[on, k, 3] = x[on]
    eng.check_status()
    state = _state(eng, n)
    env.close()
    return dict(trace=trace, nact=nact_h, counts0=counts0, state=state)


def test_trace_equals_the_per_action_calls():
    n = 4
    a = _run_a(n)
    env, acts, nact = _fresh(n)
    eng = env.engine
    trace, n_exec, done = eng.step_plans_traced(acts, nact, int(a["nact"].max()), done_explored=2.0)
    trace_h, n_exec_h, done_h, nact_h = eng.fetch(trace, n_exec, done, nact)
    np.testing.assert_array_equal(nact_h, a["nact"])  # (the same plans: the same seeds)
    np.testing.assert_array_equal(n_exec_h, a["nact"])
    assert not done_h.any()
    assert trace_h.tobytes() == a["trace"].tobytes()  # (NaN beyond the plans, in both)
    assert np.isfinite(trace_h[0, :a["nact"][0]]).all() and a["nact"].min() >= 2
    _assert_state_equal(_state(eng, n), a["state"], list(range(n)))
    env.close()


def _expected_stop(explored, nact, mid):
    """Actions executed when an env stops behind the first action whose explored share exceeds mid."""
    out = nact.copy()
    for e in range(len(nact)):
        over = np.nonzero(explored[e, :nact[e]] > mid)[0]
        if len(over):
            out[e] = over[0] + 1
    return out


def test_stop_at_done_by_the_explored_threshold():
    n = 8
    a = _run_a(n)
    ex, na = a["trace"][:, :, 3], a["nact"]
    # an env whose explored share rises between two actions inside its plan (on the CPU oracle: seed 0, 0.07 -> 0.08 at j = 0)
    found = [(e, j) for e in range(n) for j in range(na[e] - 1) if ex[e, j] < ex[e, j + 1]]
    assert found, ex
    e0, j0 = found[0]
    mid = 0.5 * (ex[e0, j0] + ex[e0, j0 + 1])
    assert ex[e0, j0] < mid < ex[e0, j0 + 1]
    env, acts, nact = _fresh(n)
    eng = env.engine
    trace, n_exec, done = eng.step_plans_traced(acts, nact, int(na.max()), done_explored=mid)
    trace_h, n_exec_h, done_h = eng.fetch(trace, n_exec, done)
    want = _expected_stop(ex, na, mid)
    assert want[e0] == j0 + 2 and n_exec_h[e0] == j0 + 2 and done_h[e0] == 1
    np.testing.assert_array_equal(n_exec_h, want)
    counts, state = _state(eng, n)
    np.testing.assert_array_equal(counts[:, 0] - a["counts0"][:, 0], want)  # the pose counts grew by the executed actions
    np.testing.assert_array_equal(counts[:, 3] - a["counts0"][:, 3], want)
    for e in range(n):
        assert trace_h[e, :want[e]].tobytes() == a["trace"][e, :want[e]].tobytes()
        assert np.isnan(trace_h[e, want[e]:]).all()  # rows beyond the stop keep their pre-fill
        assert done_h[e] == int((ex[e, :na[e]] > mid).any())
    whole = [e for e in range(n) if want[e] == na[e]]  # (among them every env whose explored stays at or below mid)
    assert all(e in whole for e in range(n) if not (ex[e, :na[e]] > mid).any())
    _assert_state_equal((counts, state), a["state"], whole)
    env.close()


def test_stop_at_done_by_the_step_limit():
    n = 4
    a = _run_a(n)
    env, acts, nact = _fresh(n)
    eng = env.engine
    step0 = a["counts0"][:, 3]
    assert (step0 == step0[0]).all() and a["nact"].min() >= 3
    trace, n_exec, done = eng.step_plans_traced(acts, nact, int(a["nact"].max()), done_explored=2.0, max_steps=int(step0[0]) + 1)
    trace_h, n_exec_h, done_h = eng.fetch(trace, n_exec, done)
    assert n_exec_h.tolist() == [2] * n and done_h.tolist() == [1] * n  # step0 + 1 is not beyond the limit, step0 + 2 is
    assert trace_h[:, :2].tobytes() == a["trace"][:, :2].tobytes() and np.isnan(trace_h[:, 2:]).all()
    assert (eng.counts_dev().cpu().numpy()[:, 0] - a["counts0"][:, 0]).tolist() == [2] * n
    # VecExplorationEnv.step_traced applies the env's own step limit (lowered here: every env stops after two actions again)
    # and adds the distance of the executed actions only
    env2, acts2, nact2 = _fresh(n)
    env2._max_steps = int(step0[0]) + 1
    _, n2, d2 = env2.step_traced(acts2, nact2)
    n2_h, d2_h, dist_h, acts_h = env2.engine.fetch(n2, d2, env2.dist, acts2)
    assert n2_h.tolist() == [2] * n and d2_h.tolist() == [1] * n and env2._graph is None
    np.testing.assert_allclose(dist_h, np.sqrt(acts_h[:, :2, 0] ** 2 + acts_h[:, :2, 1] ** 2).sum(axis=1), rtol=1e-15)
    env.close()
    env2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. the driver
# ---------------------------------------------------------------------------------------------------------------------
def _gcn(golden_dir, dev):
    from drl_graph_exploration_amd.networks import GCN
    model = GCN()
    model.load_state_dict(torch.load(os.path.join(golden_dir, "DQN_GCN_MyModel.pt"), map_location="cpu"))
    return model.to(dev).eval()


def test_driver_equals_the_hand_assembled_loop(golden_dir):
    """evaluate() over three decisions of three seeds against the loop the existing tests assemble by hand: the Q values on the
    host, np.argmax over the frontier nodes, line_plan to that frontier, one engine.step and one metrics() per action."""
    from drl_graph_exploration_amd.evaluate import evaluate
    from drl_graph_exploration_amd.networks import GraphData
    from drl_graph_exploration_amd.vecenv import VecExplorationEnv
    weights = os.path.join(golden_dir, "DQN_GCN_MyModel.pt")
    records = evaluate("DQN", "GCN", MAP, seeds=[0, 1, 2], max_decisions=3, weights=weights)
    n = 3
    env = VecExplorationEnv(MAP, n, env_index=0, test=True, n_rollouts=0)
    dev = env.device
    model = _gcn(golden_dir, dev)
    for d in range(3):
        g = env.graph_matrix()
        with torch.no_grad():
            data = GraphData(g["x"], g["edge_index"], g["edge_attr"], g["batch"], g["node_off"], g["edge_off"], g["max_graph_edges"])
            q = model(data, 0.0, batch=g["batch"]).view(-1).cpu().numpy()
        node_off, nfr, fxy = g["node_off_h"], g["n_frontier_h"], g["frontier_xy"].cpu().numpy()
        pick = [int(np.argmax(q[node_off[i + 1] - nfr[i]:node_off[i + 1]])) for i in range(n)]
        goals = np.array([fxy[i, pick[i]] for i in range(n)])
        pa, pn = env.engine.line_plan(torch.arange(n, dtype=torch.int32, device=dev), torch.as_tensor(goals, device=dev))
        pn_h = pn.cpu().numpy()
        rows = [[] for _ in range(n)]
        for k in range(int(pn_h.max())):
            env.engine.step(pa[:, k].contiguous(), (pn > k).to(torch.uint8))
            m = env.engine.metrics().cpu().numpy()
            for i in range(n):
                if k < pn_h[i]:
                    rows[i].append(m[i])
        env._graph = None
        for i in range(n):
            dec = records[i]["decisions"][d]
            assert dec["choice"] == pick[i] and dec["goal"] == goals[i].tolist()
            assert np.array(dec["plan"]).tobytes() == pa[i, :pn_h[i]].cpu().numpy().tobytes()
            assert np.array(dec["rows"]).tobytes() == np.array(rows[i]).tobytes(), (i, d)
            assert dec["time"] > 0
    env.engine.check_status()
    env.close()
    assert [r["seed"] for r in records] == [0, 1, 2] and not any(r["done"] or r["stalled"] for r in records)
    assert all(len(r["decisions"]) == 3 for r in records)


@pytest.mark.parametrize("method,model", [("A2C", "GCN"), ("DQN", "GG-NN"), ("A2C", "g-U-Net")])
def test_driver_runs_the_other_methods_and_models(method, model):
    """The soft-max branch (the frontier mask from node_off, the compact output, the prefix-sum seg_begin) and the GG-NN / g-U-Net
    trunks through evaluate(), with freshly initialised weights, two decisions of three seeds: every choice is np.argmax of the
    scores the pick saw (one per frontier of the env: the output is sized as the pick assumes), the executed rows are finite."""
    from drl_graph_exploration_amd.evaluate import build_model, evaluate
    torch.manual_seed(11)
    net = build_model(method, model)
    records = evaluate(method, model, MAP, seeds=[0, 1, 2], max_decisions=2, net=net, keep_scores=True)
    assert [r["seed"] for r in records] == [0, 1, 2]
    for rec in records:
        assert len(rec["decisions"]) == 2 and not rec["stalled"]
        for dec in rec["decisions"]:
            sc = dec["scores"]
            assert sc.dtype == np.float32 and sc.size >= 1
            assert dec["choice"] == int(np.argmax(sc))
            if method == "A2C":  # a soft-max over this env's frontiers, and over nothing else
                assert np.all(sc >= 0) and abs(float(sc.sum()) - 1.0) < 1e-4
            assert 2 <= len(dec["plan"]) and len(dec["rows"]) == len(dec["plan"]) and np.isfinite(np.array(dec["rows"])).all()


def test_driver_reproduces_the_reference_rows_free_running(golden_dir):
    """The seeds of csv_pin.json on which every pinned choice is the reference network's own pick (the selection of
    test_free_running_product_reproduces_reference_rows), through evaluate(): each seed's rows against the pinned rows at that
    test's tolerances (1e-4 relative on landmark error and trace, 2e-2 on the entropy), up to the first decision whose goal is
    not the pinned goal (1e-9) or whose plan differs from the pinned one by the documented zero-length tail action - of that
    decision the actions both plans share are still compared, then the seed leaves.  At least 150 rows must be compared (the
    hand-assembled test records 166 of 204 under the same rule); measured here: see DESIGN.md."""
    from drl_graph_exploration_amd.evaluate import evaluate
    pins = json.load(open(os.path.join(golden_dir, "csv_pin.json")))["seeds"]
    seeds = [int(k) for k, v in pins.items() if len(v["rows"]) >= 4 and
             all(isinstance(c, int) and c == g for c, g in zip(v["choices"], v["gcn_choices"]))]
    assert len(seeds) >= 5
    n_dec = max(len(pins[str(s)]["choices"]) for s in seeds)
    records = evaluate("DQN", "GCN", MAP, seeds=seeds, max_decisions=n_dec, weights=os.path.join(golden_dir, "DQN_GCN_MyModel.pt"))
    compared, bad, left = 0, [], {}
    for s, rec in zip(seeds, records):
        pin = pins[str(s)]
        row = 0
        for d, dec in enumerate(rec["decisions"]):
            if d >= len(pin["choices"]) or row >= len(pin["rows"]):
                break
            if np.any(np.abs(np.array(dec["goal"]) - np.array(pin["goals"][d])) > 1e-9):
                left[s] = ("goal", d)
                break
            want, mine = np.array(pin["plans"][d]).reshape(-1, 3), np.array(dec["plan"]).reshape(-1, 3)
            k0 = min(len(want), len(mine))
            assert np.allclose(mine[:k0], want[:k0], atol=1e-7), (s, d, want, mine)
            n_cmp = len(dec["rows"])
            if len(want) != len(mine):
                last_cut = pin["finished"] and d + 1 == len(pin["choices"])  # (the reference's episode ended inside this plan)
                if not (last_cut and len(want) < len(mine)):
                    assert abs(len(want) - len(mine)) == 1 and np.allclose((want if len(want) > k0 else mine)[k0:], 0.0, atol=1e-7), \
                        (s, d, want, mine)
                    left[s] = ("tail", d, len(want), len(mine))
                n_cmp = min(n_cmp, k0)
            for k in range(n_cmp):
                if row >= len(pin["rows"]):
                    break
                ref = np.array(pin["rows"][row])
                rel = np.abs(np.array(dec["rows"][k]) - ref) / np.abs(ref)
                if rel[0] > 1e-4 or rel[2] > 1e-4 or rel[1] > 2e-2:
                    bad.append((s, row, rel.tolist()))
                row += 1
                compared += 1
            if s in left:
                break
    print("free-running driver: %d rows compared over seeds %s, left at %s" % (compared, seeds, left))
    assert not bad, bad[:5]
    assert compared >= 150, (compared, left)
