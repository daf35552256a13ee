"""The cases of tests/rect_cases.py checked on the CPU, with the oracle and numpy only, before tests/test_gpu_rect.py uses them.
Every assertion here is a condition on the INPUTS of the GPU tests (shapes, where the trajectories go, that nothing sits on a knife
edge, that the probes and the worlds tell x from y), not a measurement of the code under test.  No GPU."""
import math

import numpy as np
import pytest

import em_ref
import em_tree_cases as K
import em_tree_ref as R
import og_ref
import rect_cases as RC
from graph_checks import oracle_graph
from oracle import fm2_ref
from oracle import oracle as O
from test_og_cpu import GEOMETRY_MARGIN, THRESH_MARGIN

EM_MARGIN = 1e-9  # tests/test_em_cpu.py: test_no_parity_case_sits_on_a_knife_edge


def _run(name, cfg_name=None):
    """The world's sims stepped through its script; per step the knife-edge cell count of every env."""
    sims = RC.fresh_sims(name, cfg_name)
    knife = []
    for act in RC.script_of(name):
        for s in sims:
            assert s.simulate(act) == 0
        knife.append([int(s.knife_edge_cells(1e-9).sum()) for s in sims])
    return sims, knife


@pytest.fixture(scope="module")
def runs():
    return {name: _run(name) for name in RC.WORLDS}


def test_grids_are_rectangles_with_four_distinct_bounds(runs):
    for name, (sims, _) in runs.items():
        c = sims[0].cfg
        assert sims[0].vm_shape() == RC.SHAPES[name]
        assert len({c.map_min_x, c.map_max_x, c.map_min_y, c.map_max_y}) == 4
        rows, cols = sims[0].vm_shape()
        assert rows != cols and rows % 8 != 0 and cols % 8 != 0 and rows % 8 != cols % 8
    assert RC.SHAPES["wide"] == (23, 27) and RC.SHAPES["tall"] == (27, 23) and 23 * 27 == 621
    assert RC.window(runs["wide"][0][0].cfg) == 7 and RC.window(runs["win8"][0][0].cfg) == 8
    assert len(RC.SCRIPT) <= 24 and RC.SCRIPT[:4] == RC.RESET


def test_no_compared_step_has_a_knife_edge_cell(runs):
    for name, (_, knife) in runs.items():
        assert not np.any(knife), name


@pytest.mark.parametrize("name", ["wide", "tall", "sector"])
def test_trajectories_reach_the_ragged_tiles_and_all_four_grid_edges(runs, name):
    sims, _ = runs[name]
    cfg = sims[0].cfg
    rows, cols = sims[0].vm_shape()
    W = RC.window(cfg)
    edges, cells = set(), []
    for s in sims:
        assert s.num_landmarks() >= 5  # landmarks are seen (from the reset on: OracleEnv would otherwise draw another world)
        for x, y, _ in s.poses()[0]:
            r, c = RC.cell_of(cfg, x, y)
            assert 0 <= r < rows and 0 <= c < cols  # (the vehicle stays on the grid: OracleEnv.graph_matrix indexes its cell)
            cells.append((r, c))
            r0, c0 = RC.window_origin(cfg, x, y)
            edges |= {k for k, over in (("bottom", r0 < 0), ("left", c0 < 0), ("top", r0 + W > rows), ("right", c0 + W > cols)) if over}
    # beyond the OTHER extent: an index that exchanged rows and cols would fall off the grid or into another row
    if RC.WORLDS[name]["box"] == "wide":
        assert max(c for _, c in cells) >= 23
    else:
        assert max(r for r, _ in cells) >= 23
    assert edges == {"bottom", "left", "top", "right"}


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_every_probe_tells_the_x_bounds_from_the_y_bounds(name):
    cfg = RC.oracle_config(name)
    verdicts = []
    for start, odom in RC.PROBES[name]:
        sim = O.OracleSim(cfg, 0, 0, start=start)
        rejected = sim.simulate(odom) == 1
        assert rejected == (not RC.accepts(cfg, odom)) and rejected == RC.accepts(cfg, odom, swapped=True)
        assert sim.num_poses() == (1 if rejected else 2)
        x, y, _ = sim.poses()[0][-1]
        assert cfg.map_min_x < x < cfg.map_max_x and cfg.map_min_y < y < cfg.map_max_y
        verdicts.append(rejected)
    assert sorted(verdicts) == [False, False, True, True]


# envs whose run under the OTHER world's boxes ends without a frontier cell in the interior box (the reference then indexes an empty list)
NO_FRONTIER_TRANSPOSED = {"wide": [2], "tall": [1]}


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_the_transposed_configuration_gives_another_answer(runs, name):
    """Same starts, same (whole) script, the other world's boxes: were x and y mixed up somewhere, the two runs could agree."""
    sims, _ = runs[name]
    other, _ = _run(name, RC.TRANSPOSE[name])
    envs = [RC.make_envs(name), [O.OracleEnv(14, i, num_landmarks=RC.NUM_LANDMARKS, start=tuple(RC.STARTS[name][i]),
                                              cfg=RC.oracle_config(RC.TRANSPOSE[name])) for i in range(RC.N_ENVS)]]
    for g, group in enumerate(envs):
        for i, env in enumerate(group):
            for act in RC.SCRIPT[4:]:
                env.step(act)
            if g == 1 and i in NO_FRONTIER_TRANSPOSED[name]:
                with pytest.raises(TypeError):
                    env.frontier()
                assert env.all_frontiers == []
            else:
                env.frontier()
                assert env.all_frontiers
    for i in range(RC.N_ENVS):
        a, b = sims[i].virtual_map()[0], other[i].virtual_map()[0]
        assert a.shape == b.shape[::-1] and not np.array_equal(a, b.T)
        assert sims[i].calculate_utility(0.0) != other[i].calculate_utility(0.0)
        assert sorted(map(tuple, envs[0][i].all_frontiers)) != sorted(map(tuple, envs[1][i].all_frontiers))


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_every_env_has_a_frontier_after_the_script(name):
    envs = RC.make_envs(name)
    for env in envs:
        for act in RC.SCRIPT[4:]:
            env.step(act)
        og = oracle_graph(env)
        assert og["F"] >= 1 and og["N"] == env._sim.key_size() + og["F"]
        assert env._sim.vm_shape() == RC.SHAPES[name] and env.env_index < RC.N_ENVS  # (the given configuration, no other world drawn)


def test_the_chunk_loop_stays_in_the_vehicle_box_and_masks_nothing():
    cfg = RC.oracle_config("wide")
    sims = [O.OracleSim(cfg, i, i, start=tuple(RC.CHUNK_STARTS[i])) for i in range(2)]
    seen = []
    for s in range(RC.CHUNK_STEPS):
        for sim in sims:
            assert sim.simulate(RC.CHUNK_LOOP[s % len(RC.CHUNK_LOOP)]) == 0
        if s in RC.CHUNK_CHECKS:
            seen.append(sims[0].num_poses())
            assert not any(sim.knife_edge_cells().any() for sim in sims)
    assert seen == [64, 65, 67]
    for sim in sims:
        xy = sim.poses()[0]
        for p in (xy, np.array([sim.ground_truth()[0]])):  # the estimated trajectory, and where the vehicle really ends
            assert cfg.env_min_x < p[:, 0].min() and p[:, 0].max() < cfg.env_max_x
            assert cfg.env_min_y < p[:, 1].min() and p[:, 1].max() < cfg.env_max_y


def test_the_8_cell_window_holds_41_cells_in_range():
    """Per pose the cell centres nearer than max_range = 7 m = 3.5 cells.  At the chosen spots the first poses (turns in place)
    count 41 each - more than the 40 per pose the compact stage of the map kernel is carved for: the pair list of env 0's
    first rebuilds is longer than 40 P."""
    cfg = RC.oracle_config("win8")
    # the lattice count itself: an open disc of radius 3.5 around a point 0.28 cell off a lattice point along one axis
    k = np.arange(-6, 7)
    KX, KY = np.meshgrid(k, k)
    assert int(np.sum(KX ** 2 + (KY - 0.28) ** 2 < 3.5 ** 2)) == 41 and int(np.sum((KX - 0.31) ** 2 + (KY - 0.17) ** 2 < 3.5 ** 2)) < 41
    sims = RC.fresh_sims("win8")
    over = {i: [] for i in range(RC.N_ENVS)}
    for s, act in enumerate(RC.SCRIPT_WIN8):
        for i, sim in enumerate(sims):
            assert sim.simulate(act) == 0
            n = RC.in_range_cells(sim)
            assert max(n) <= 41
            if sum(n) > 40 * len(n):
                over[i].append(s)
    print("steps whose pair list exceeds 40 per pose: %s; in-range cells per pose at the end: %s" % (over, [RC.in_range_cells(s) for s in sims]))
    assert over[0][:3] == [0, 1, 2] and over[2][:2] == [0, 1] and over[1] == []  # envs 0, 2 from the first rebuild (P = 2) on; the generic spot never
    assert max(RC.in_range_cells(sims[0])) == max(RC.in_range_cells(sims[2])) == 41 and max(RC.in_range_cells(sims[1])) < 41


def _lattice_max(r, n=100):
    """The largest count of lattice points within r of a centre, over an n x n net of centres in [0, 1/2]^2: a lower bound of the
    true maximum (brute force, numpy)."""
    k = np.arange(-int(math.ceil(r)) - 1, int(math.ceil(r)) + 2)
    KX, KY = np.meshgrid(k, k)
    u = (np.arange(n) + 0.5) * (0.5 / n)
    d2 = (KX[None, None] - u[:, None, None, None]) ** 2 + (KY[None, None] - u[None, :, None, None]) ** 2
    return int((d2 < r * r).sum(axis=(2, 3)).max())


def test_the_hosts_lattice_bound_against_brute_force():
    """drlgx_debug_disc_cells_bound - what decides whether the map kernel's compact form may serve a sensor - is an upper bound of
    the lattice count at every radius a window admits, and no looser than the count at a radius 0.02 cell larger: its own net widens
    the radius by 1 / (64 sqrt 2) = 0.01105 and the net here (side 1 / 200) has a covering radius of 0.0036.  Exact where it matters:
    32 at 3.0 cells (the default sensor: compact form kept), 41 at 3.5 (the 8-cell window: more than kPairsPerPose = 40)."""
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    for r in (0.5, 1.0, 1.5, 2.0, 2.25, 2.5, 2.75, 3.0, 3.1, 3.25, 3.3, 3.4, 3.45, 3.5):
        got = L.drlgx_debug_disc_cells_bound(r)
        assert _lattice_max(r) <= got <= _lattice_max(r + 0.02), r
    assert L.drlgx_debug_disc_cells_bound(3.0) == 32 == _lattice_max(3.0) and L.drlgx_debug_disc_cells_bound(3.5) == 41 == _lattice_max(3.5)


@pytest.mark.parametrize("name", ["wide", "tall", "sector"])
def test_cost_plans_keep_their_margins(runs, name):
    sims, _ = runs[name]
    worst = {"range": math.inf, "bearing": math.inf, "floor": math.inf, "thresh": math.inf}
    worst_em = math.inf
    for sim in sims:
        plans = RC.plans_for(sim)
        assert [len(p) for p in plans[:3]] == [0, 1, RC.MAX_ACTIONS] and len(plans[3]) <= RC.MAX_ACTIONS
        import og_cases
        assert og_cases.leaves_the_map(sim, plans[3])
        for plan in plans:
            margins = og_ref.og_cost(sim, plan)[3]
            for key in worst:
                worst[key] = min(worst[key], margins[key])
        em_plans = RC.em_plans_for(sim)
        assert [len(p) for p in em_plans] == [len(p) for p in plans]  # (nothing was cut: the spiral keeps its max_actions)
        for plan in em_plans:
            assert sum(fm2_ref.fm2_update(sim, plan)[1]) <= 256
            worst_em = min(worst_em, min(em_ref.em_cost(sim, plan, 0)[3].values()))
    print("%s: og margins %s, em margin %.3e" % (name, ", ".join("%s %.3e" % kv for kv in sorted(worst.items())), worst_em))
    assert min(worst["range"], worst["bearing"], worst["floor"]) > GEOMETRY_MARGIN
    assert worst["thresh"] > THRESH_MARGIN
    assert worst_em > EM_MARGIN


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_trees_have_their_nearest_node_margins(runs, name):
    """The margin that entitles the GPU test to exact parent indices, from the oracle's root pose (the engine's is 1e-9 away)."""
    sims, _ = runs[name]
    cfg = sims[0].cfg
    for env, sim in enumerate(sims):
        root = sim.poses()[0][-1]
        t = K.tree_of(cfg, root, K.START_INDICES[env], n_accept=RC.TREE_NODES)
        assert len(t) == RC.TREE_NODES + 1 and max(t.depth) <= RC.MAX_ACTIONS and min(t.margin) > 1e3 * K.MARGIN
        xy = t.xytheta()
        assert np.ptp(xy[:, 0]) > 0 and np.ptp(xy[:, 1]) > 0
        g = K.tree_of(cfg, root, K.START_INDICES[env], goal=tuple(RC.RRT_GOALS[name][env]))
        assert g.result == R.SUCCESS and min(g.margin) > 1e3 * K.MARGIN and 3 < g.depth[g.goal_node] <= RC.MAX_ACTIONS
