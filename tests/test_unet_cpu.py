"""CPU tests of the g-U-Net modules (scripts/Networks.py:125-449): construction, `state_dict` layout and init without a GPU, checkpoint
exchange with the plain-torch restatement, the refused constructor arguments, and the restatement itself on a case done by hand; the cases of
tests/test_gpu_unet_edges.py (tests/unet_cases.py): the regime each reaches, the sparse augment reference against the dense one, the
score gaps of the trunk cases."""
import io
import math

import pytest
import torch

import test_gpu_unet as TU
import unet_cases as UC
import unet_ref


def expected_keys(depth, hidden, in_dim, out_dim):
    keys = []
    for i in range(depth + 1):
        keys += [("down_convs.%d.weight" % i, (in_dim if i == 0 else hidden, hidden)), ("down_convs.%d.bias" % i, (hidden,))]
    keys += [("pools.%d.weight" % i, (1, hidden)) for i in range(depth)]
    for i in range(depth):
        keys += [("up_convs.%d.weight" % i, (hidden, hidden)), ("up_convs.%d.bias" % i, (hidden,))]
    return keys + [("fully_con1.weight", (out_dim, hidden)), ("fully_con1.bias", (out_dim,))]


@pytest.mark.parametrize("name,out_dim", [("GraphUNet", 1), ("PolicyGraphUNet", 1), ("ValueGraphUNet", 100)])
def test_modules_construct_on_the_cpu_with_the_reference_layout(name, out_dim):
    from drl_graph_exploration_amd import networks
    torch.manual_seed(0)
    m = getattr(networks, name)(5, 1000, 1000, 3)  # the reference's call (scripts/train.py:44-45, 71-72)
    sd = m.state_dict()
    want = expected_keys(3, 1000, 5, out_dim)
    assert list(sd.keys()) == [k for k, _ in want] and len(want) == 19
    for k, shape in want:
        assert tuple(sd[k].shape) == shape and sd[k].dtype == torch.float32, k
    for k, v in sd.items():
        if k.endswith("bias") and "conv" in k:
            assert bool((v == 0).all()), k  # GCNConv: zeros
        elif "conv" in k:
            bound = math.sqrt(6.0 / (v.shape[0] + v.shape[1]))  # glorot
            assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.95 * bound and abs(float(v.mean())) < 0.1 * bound, k
        else:  # pools (PyG's `uniform(size, tensor)`) and Linear(1000, out): +-1/sqrt(1000)
            bound = 1.0 / math.sqrt(1000.0)
            assert float(v.abs().max()) <= bound, k
            if v.numel() >= 1000:
                assert float(v.abs().max()) > 0.95 * bound and abs(float(v.mean())) < 0.1 * bound, k
    assert [tuple(p.shape) for p in m.trunk_parameters()] == [s for _, s in want]
    assert m.depth == 3 and m.pool_ratios == [0.5, 0.5, 0.5]
    small = getattr(networks, name)(5, 8, 8, 1, pool_ratios=0.8)
    assert list(small.state_dict().keys()) == [k for k, _ in expected_keys(1, 8, 5, out_dim)]


def test_a_plain_torch_checkpoint_loads_strictly():
    from drl_graph_exploration_amd import networks
    torch.manual_seed(1)
    for cls, out_dim in ((networks.GraphUNet, 1), (networks.PolicyGraphUNet, 1), (networks.ValueGraphUNet, 100)):
        ref = unet_ref.RefGraphUNet(5, 1000, 3, 0.5, out_dim)
        buf = io.BytesIO()
        torch.save(ref.state_dict(), buf)
        buf.seek(0)
        m = cls(5, 1000, 1000, 3)
        m.load_state_dict(torch.load(buf, map_location="cpu"), strict=True)
        for a, b in zip(m.trunk_parameters(), ref.trunk_parameters()):
            assert torch.equal(a, b)
        ref.load_state_dict(m.state_dict(), strict=True)


def test_what_the_hip_path_does_not_do_is_refused_at_construction():
    from drl_graph_exploration_amd.networks import GraphUNet, PolicyGraphUNet, ValueGraphUNet
    for cls in (GraphUNet, PolicyGraphUNet, ValueGraphUNet):
        with pytest.raises(ValueError):
            cls(5, 8, 8, 2, sum_res=False)
        with pytest.raises(ValueError):
            cls(5, 8, 8, 2, act=torch.tanh)
        for depth in (0, 5, -1):
            with pytest.raises(ValueError):
                cls(5, 8, 8, depth)
        with pytest.raises(ValueError):
            cls(5, 8, 8, 2, pool_ratios=[0.5, 0.8])
        with pytest.raises(ValueError):
            cls(5, 8, 12, 2)
        cls(5, 8, 8, 4)


def test_there_is_no_cpu_fallback():
    from drl_graph_exploration_amd import networks
    from drl_graph_exploration_amd._lib import DrlgxError
    data = networks.GraphData(torch.zeros(2, 5), torch.tensor([[0], [1]]), torch.ones(1))
    for cls in (networks.GraphUNet, networks.PolicyGraphUNet, networks.ValueGraphUNet):
        with pytest.raises(DrlgxError):
            cls(5, 8, 8, 1)(data, 0.0 if cls is networks.GraphUNet else torch.ones(2, dtype=torch.bool))
    with pytest.raises(DrlgxError):
        networks.unet_forward_raw(data.x, data.edge_index, data.edge_attr, networks.GraphUNet(5, 8, 8, 1).trunk_parameters(), 1)


def test_restatement_on_the_path_done_by_hand():
    """0 -> 1 -> 2 with weights 2 and 3.  (A + I)^2 = A^2 + 2 A + I: (0,1) = 2 * 2, (1,2) = 2 * 3, (0,2) = 2 * 3, nothing else off
    the diagonal.  p = e_0 and first features (0.5, -1, 2): scores tanh of those, k = ceil(0.5 * 3) = 2 keeps nodes 0 and 2, so the
    pooled graph has the one entry (0, 1) = 6 and the gates are tanh(0.5), tanh(2)."""
    ei, ea = torch.tensor([[0, 1], [1, 2]]), torch.tensor([2.0, 3.0], dtype=torch.float64)
    full, w, counts = unet_ref.augment_filter(ei, ea, [3], torch.arange(3), [3])
    assert sorted(zip(full[0].tolist(), full[1].tolist(), w.tolist())) == [(0, 1, 4.0), (0, 2, 6.0), (1, 2, 6.0)] and counts == [3]
    pool = unet_ref.TopKPooling(4).double()
    with torch.no_grad():
        pool.weight.copy_(torch.tensor([[3.0, 0.0, 0.0, 0.0]]))  # any multiple of e_0: the score divides by |p|
    x = torch.tensor([[0.5, 9, 9, 9], [-1.0, 9, 9, 9], [2.0, 9, 9, 9]], dtype=torch.float64)
    s = pool.score(x)
    assert torch.allclose(s, torch.tanh(torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64)), rtol=0, atol=1e-15)
    assert unet_ref.keep_count(3, 0.5) == 2 and unet_ref.keep_count(1, 0.5) == 1 and unet_ref.keep_count(5, 0.8) == 4
    perm, gaps = unet_ref.select(s.detach(), [3], 0.5)
    assert perm.tolist() == [0, 2]
    assert gaps[0] == pytest.approx(math.tanh(0.5) - math.tanh(-1.0))
    sub, sw, _ = unet_ref.augment_filter(ei, ea, [3], perm, [2])
    assert sub.tolist() == [[0], [1]] and sw.tolist() == [6.0]
    gated = x[perm] * s[perm].unsqueeze(1)
    assert torch.allclose(gated[:, 0], torch.tensor([0.5 * math.tanh(0.5), 2.0 * math.tanh(2.0)], dtype=torch.float64))
    # ties go to the lower index; a graph of one node stays one node; level sizes follow from ceil
    perm, gaps = unet_ref.select(torch.tensor([1.0, 1.0, 1.0, 0.5, 7.0]), [4, 1], 0.5)
    assert perm.tolist() == [0, 1, 4] and gaps == [0.0, math.inf]
    assert unet_ref.level_sizes([5, 1, 11, 2], 0.5, 3) == [[5, 1, 11, 2], [3, 1, 6, 1], [2, 1, 3, 1], [1, 1, 2, 1]]


def test_restatement_trunk_runs_and_every_parameter_gets_a_gradient():
    torch.manual_seed(2)
    m = unet_ref.RefGraphUNet(5, 8, 2, 0.5, 3).double()
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(9, 5, generator=gen, dtype=torch.float64)
    ei = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7, 0, 3], [1, 2, 3, 4, 0, 6, 7, 8, 2, 1]])
    ea = torch.rand(10, generator=gen, dtype=torch.float64) + 0.1
    out = m(x, ei, ea, None, [5, 4])
    assert out.shape == (9, 3) and bool(torch.isfinite(out).all())
    assert [lv["sizes"] for lv in m.levels] == [[3, 2], [2, 1]]
    out.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert float(m.pools[0].weight.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_unet_edges.py: what they reach, their reference and their preconditions
# ---------------------------------------------------------------------------------------------------------------------
def same_entries(a, b):
    return a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2] == b[2]


def test_the_regime_formulas_on_the_figures_worked_by_hand():
    """T = min(256, (lds_words - n) / (2 n + 2 ceil(n / 32))) with the whole budget: below the node count from 126 nodes, 64 -> 63 at
    246 -> 247, 78 at 200, 15 at 1 025, 3 at the cap; a 61-node graph beside a 200-node one has 256 rows, a 62-node one 255."""
    assert UC.launch_lds_words(71, 71) == 71 + 71 * (142 + 6) and UC.launch_lds_words(126, 126) == UC.LDS_WORDS
    full = [UC.rows_in_flight(n, UC.LDS_WORDS) for n in (125, 126, 200, 246, 247, 1025, 4095, 4096)]
    assert full == [126, 125, 78, 64, 63, 15, 3, 3]
    assert UC.regime([125], [125], 125) == [(125, 1)]  # (its own launch asks for 125 rows only)
    assert UC.regime([4096], [7], 4096) == [(3, 3)] and UC.regime([61, 62, 200], [61, 62, 200], 200) == [(256, 1), (255, 1), (78, 3)]


@pytest.mark.parametrize("case", UC.AUGMENT_CASES, ids=UC.AUGMENT_IDS)
def test_augment_cases_reach_their_regime_and_the_sparse_reference_equals_the_dense_one(case):
    inp = UC.augment_inputs(case)
    expect = [case["expect"][j] for j in inp["order"]]
    assert UC.regime(inp["sizes"], inp["ks"], inp["max_nodes"]) == expect
    assert max(inp["sizes"]) <= inp["max_nodes"] <= UC.MAX_GRAPH_NODES
    ei, ew, counts, largest = UC.augment_reference(inp)
    assert 0 < largest < UC.EXACT_LIMIT  # float32 sums of these integers are exact
    assert bool((ew == ew.round()).all())
    if max(inp["sizes"]) <= UC.DENSE_REF_NODES:
        assert same_entries((ei, ew, counts), UC.augment_reference(inp, dense=True))
    for (kind, n, keep), k, c in zip([case["graphs"][j] for j in inp["order"]], inp["ks"], counts):
        assert c <= k * (k - 1)
        if kind == "star":
            assert c == k * (k - 1) and k == n  # the dense product: no free slot
    if case.get("foreign"):
        used = inp["edge_index"][:, :inp["used"]]
        assert int((used == -1).all(0).sum()) >= 40 and inp["edge_index"].shape[1] > inp["used"]
        g0 = used[:, :int(inp["edge_off"][1])]
        assert int(((g0[0] >= 200) ^ (g0[1] >= 200)).sum()) == 12  # one endpoint in the neighbouring graph


def test_boundary_halves_hold_or_lack_both_sides_of_each_word_boundary():
    for n in (33, 65, 97):
        for keep, inside in (("with", True), ("without", False)):
            kept = UC.kept_rows(n, keep, torch.Generator().manual_seed(n)).tolist()
            assert len(kept) == (n + 1) // 2 and kept == sorted(set(kept))
            assert all((c in kept) == inside for c in UC.BOUNDARY_COLUMNS if c < n)


def test_mixed_batch_reversed_holds_the_same_graphs():
    fwd, rev = (UC.augment_inputs(c) for c in UC.AUGMENT_CASES if c["id"] in ("mixed", "mixed-reversed"))
    assert rev["sizes"] == fwd["sizes"][::-1] and rev["order"] == fwd["order"][::-1]
    for j in range(len(fwd["sizes"])):
        g = len(fwd["sizes"]) - 1 - j
        a = fwd["edge_index"][:, int(fwd["edge_off"][j]):int(fwd["edge_off"][j + 1])] - int(fwd["node_off"][j])
        b = rev["edge_index"][:, int(rev["edge_off"][g]):int(rev["edge_off"][g + 1])] - int(rev["node_off"][g])
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["fan", "star_in", "star_out", "star_both", "star_drop_hub", "isolated", "duplicates", "batch"])
def test_sparse_reference_equals_the_dense_one_on_the_existing_cases(kind):
    gen = torch.Generator().manual_seed(17)
    sizes, ei, ew, perm = TU.augment_case(kind, gen)
    if perm is None:
        perm, _ = unet_ref.select(torch.rand(sum(sizes), generator=gen), sizes, 0.5)
        ks = [unet_ref.keep_count(n, 0.5) for n in sizes]
    else:
        ks = [int(perm.numel())]
    assert same_entries(unet_ref.augment_filter_sparse(ei, ew.double(), sizes, perm, ks), unet_ref.augment_filter(ei, ew.double(), sizes, perm, ks))


@pytest.mark.parametrize("case", UC.TRUNK_CASES, ids=UC.TRUNK_IDS)
def test_trunk_cases_keep_every_kth_place_clear(case):
    """The precondition of the GPU comparison, on the float64 reference alone: a case that loses its gap fails here first."""
    _, kind, hidden, depth, out_dim, with_mask, ratio, seed = case
    model, x, ei, ea, sizes, mask, d_out = UC.trunk_case(kind, hidden, depth, out_dim, with_mask, ratio, seed)
    m = unet_ref.RefGraphUNet(5, hidden, depth, ratio, out_dim).double()
    m.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    with torch.no_grad():
        m(x.double(), ei, ea.double(), None, sizes)
    assert TU.GAP == 1e-3 and len(m.levels) == depth
    TU.assert_gaps(m.levels)
    want = unet_ref.level_sizes([x.shape[0]] if sizes is None else sizes, ratio, depth)
    assert [lv["sizes"] for lv in m.levels] == want[1:]
    if kind == "n200":
        assert [s[0] for s in want] == [200, 160, 128, 103, 83]
    if kind == "mixed":
        assert max(sizes) > 125 and 1 in sizes
    if ratio == 1.0:  # every node kept at every level: the identity
        assert all(lv["perm"].tolist() == list(range(x.shape[0])) and min(lv["gaps"]) == math.inf for lv in m.levels)


def test_module_case_at_depth_4_keeps_every_kth_place_clear():
    from drl_graph_exploration_amd.networks import GraphUNet
    x, ei, ea, sizes, _ = TU.module_batch()
    torch.manual_seed(UC.MODULE_SEED)
    model = GraphUNet(5, 1000, 1000, 4)
    m64, _ = TU.module_reference(model, x, ei, ea, None, None, sizes, torch.float64)
    assert len(m64.levels) == 4 and len(list(model.parameters())) == 24
    TU.assert_gaps(m64.levels)
