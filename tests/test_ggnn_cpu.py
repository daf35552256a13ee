"""CPU tests of the GG-NN modules (scripts/Networks.py:73-122): construction, `state_dict` layout and init without a GPU, the
reference's checkpoints' keys, and the trainers' model factory; then the cases of tests/test_gpu_ggnn_edges.py (tests/ggnn_cases.py):
the regime each reaches, its distance from the ReLU's kink, and the dense restatement of the aggregation against the `index_add_` one."""
import io
import math

import pytest
import torch

import ggnn_cases as GC
import ggnn_ref

KEYS = {
    "gconv1.weight": (3, 1000, 1000),
    "gconv1.rnn.weight_ih": (3000, 1000),
    "gconv1.rnn.weight_hh": (3000, 1000),
    "gconv1.rnn.bias_ih": (3000,),
    "gconv1.rnn.bias_hh": (3000,),
    "fully_con1.weight": None,  # (out, 1000)
    "fully_con1.bias": None,
}


@pytest.mark.parametrize("name,out_dim", [("GGNN", 1), ("PolicyGGNN", 1), ("ValueGGNN", 100)])
def test_modules_construct_on_the_cpu_with_the_reference_layout(name, out_dim):
    from drl_graph_exploration_amd import networks
    torch.manual_seed(0)
    m = getattr(networks, name)()
    sd = m.state_dict()
    assert list(sd.keys()) == list(KEYS.keys())
    for k, shape in KEYS.items():
        want = shape if shape is not None else ((out_dim, 1000) if k.endswith("weight") else (out_dim,))
        assert tuple(sd[k].shape) == want and sd[k].dtype == torch.float32, k
    # init: weight and the GRU cell uniform in +-1/sqrt(1000) (PyG's `uniform(size, tensor)`, torch's GRUCell.reset_parameters), and
    # actually spread over that range; Linear(1000, out): +-1/sqrt(1000) too
    bound = 1.0 / math.sqrt(1000.0)
    for k, v in sd.items():
        assert float(v.abs().max()) <= bound, k
        if v.numel() >= 1000:
            assert float(v.abs().max()) > 0.95 * bound and abs(float(v.mean())) < 0.1 * bound, k
    assert [tuple(p.shape) for p in m.trunk_parameters()] == [tuple(sd[k].shape) for k in KEYS]
    assert len(list(m.parameters())) == 7  # (FusedAdam's limit is eight tensors)


def test_a_plain_torch_checkpoint_loads_strictly():
    """A `state_dict` saved from a plain-torch module that holds a real GRUCell under `gconv1.rnn` (what the reference's
    Networks.GGNN saves through PyG's GatedGraphConv) loads into the HIP-backed classes with strict=True, and back."""
    from drl_graph_exploration_amd import networks
    torch.manual_seed(1)
    for cls, out_dim in ((networks.GGNN, 1), (networks.PolicyGGNN, 1), (networks.ValueGGNN, 100)):
        ref = ggnn_ref.RefGGNN(1000, 3, out_dim)
        buf = io.BytesIO()
        torch.save(ref.state_dict(), buf)
        buf.seek(0)
        m = cls()
        m.load_state_dict(torch.load(buf, map_location="cpu"), strict=True)
        for a, b in zip(m.trunk_parameters(), ref.trunk_parameters()):
            assert torch.equal(a, b)
        ref.load_state_dict(m.state_dict(), strict=True)


def test_there_is_no_cpu_fallback():
    from drl_graph_exploration_amd import networks
    from drl_graph_exploration_amd._lib import DrlgxError
    data = networks.GraphData(torch.zeros(2, 5), torch.tensor([[0], [1]]), torch.ones(1))
    with pytest.raises(DrlgxError):
        networks.GGNN()(data, 0.0)


def test_model_factory_knows_both_families_and_still_refuses_g_u_net():
    from drl_graph_exploration_amd import networks
    from drl_graph_exploration_amd.train import make_models, paths
    cpu = torch.device("cpu")
    q, tgt = make_models("DQN", "GG-NN", cpu)
    assert type(q) is networks.GGNN and type(tgt) is networks.GGNN and q is not tgt
    actor, critic = make_models("A2C", "GG-NN", cpu)
    assert type(actor) is networks.PolicyGGNN and type(critic) is networks.ValueGGNN
    assert type(make_models("DQN", "GCN", cpu)[0]) is networks.GCN
    assert paths("d", "DQN", "GG-NN")[0] == "DQN_GG-NN/" and paths("d", "A2C", "GG-NN")[0] == "A2C_GG-NN/"
    with pytest.raises(NotImplementedError) as err:
        make_models("DQN", "g-U-Net", cpu)
    assert "g-U-Net" in str(err.value) and "GG-NN /" not in str(err.value)


def test_restatement_aggregates_at_the_target_node():
    """The checker itself on a case small enough to do by hand: one layer, hidden 2, identity weight, edge 0 -> 1 with weight 3:
    only node 1 receives (3 x node 0's state), so its GRU input differs from zero and node 0's does not."""
    conv = ggnn_ref.GatedGraphConv(2, 1).double()
    with torch.no_grad():
        conv.weight[0] = torch.eye(2)
    x = torch.tensor([[1.0, 2.0], [5.0, 7.0]], dtype=torch.float64)
    h = conv(x, torch.tensor([[0], [1]]), torch.tensor([3.0], dtype=torch.float64))
    want0 = conv.rnn(torch.zeros(1, 2, dtype=torch.float64), x[0:1])
    want1 = conv.rnn(3.0 * x[0:1], x[1:2])
    assert torch.allclose(h[0:1], want0) and torch.allclose(h[1:2], want1)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_ggnn_edges.py: their regimes, their distance from the ReLU's kink, and the checker itself
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, ref):
    d, m = float((a - ref).abs().max()) if ref.numel() else 0.0, float(ref.abs().max()) if ref.numel() else 0.0
    return d / m if m > 0 else (0.0 if d == 0 else math.inf)


@pytest.mark.parametrize("cid", GC.IDS)
def test_edge_case_reaches_the_regime_its_table_row_says(cid):
    case = GC.BY_ID[cid]
    with_segments, generic = GC.expected(case)
    assert GC.regime(case, False) == generic
    if case["ways"] == "both":
        assert GC.regime(case, True) == with_segments
    sizes, counts = GC.graph_sizes(case)
    ei, ea, kind = GC.edges(case)
    assert ei.shape == (2, sum(counts)) and ea.shape == (sum(counts),)
    # grouped by graph: every live edge inside its graph's nodes, every cross edge with exactly one endpoint outside, dead slots (-1, -1)
    node_off = torch.tensor([0] + sizes).cumsum(0)
    slot_graph = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(counts))
    lo, hi = node_off[slot_graph], node_off[slot_graph + 1]
    inside = (ei >= lo) & (ei < hi)
    assert bool(inside[:, kind == 0].all()) and bool((inside[:, kind == 2].sum(0) == 1).all()) and bool((ei[:, kind == 1] == -1).all())
    assert bool(((ei[:, kind == 2] >= 0) & (ei[:, kind == 2] < sum(sizes))).all())  # (in range: the generic build would keep them)
    assert 1 <= case["layers"] <= GC.MAX_LAYERS and case["in_dim"] <= min(8, case["hidden"]) and case["hidden"] % 4 == 0
    loops = ei[0] == ei[1]
    assert torch.unique(ei[0][loops & (kind == 0)]).numel() == int((loops & (kind == 0)).sum())  # never two self loops on one node


def test_edge_case_table_covers_what_it_claims():
    reg = {c["id"]: (GC.regime(c, c["ways"] == "both"), c) for c in GC.CASES}
    one = [r for r, c in reg.values() if r["build"] == "one-launch"]
    passes = [p for r in one for p in r["csr"]]
    assert {p[0] for p in passes} >= {0, 1, 2, 3} and {p[1] for p in passes} >= {0, 1, 2, 3, 8}
    assert [GC.graph_sizes(c)[1][0] - GC.RAW_MAX_EDGES for _, c in reg.values() if c["id"].startswith("A3-e")] == [-1, 0, 1]
    assert reg["A3-e2048"][0]["build"] == "one-launch" and reg["A3-e2049"][0]["build"] == "generic" and reg["A3-5+11+e2049"][0]["build"] == "generic"
    assert {r["scan"] for r, c in reg.values() if "scan" in r} >= {1, 2, 3}
    assert (128, 8) in {r["thin"] for r, _ in reg.values()} and {r["splitk"] for r, _ in reg.values()} >= {1, 2, 8}
    assert {c["in_dim"] for c in GC.CASES} == {1, 3, 4, 5, 8} and {c["layers"] for c in GC.CASES} >= {4, 5, GC.MAX_LAYERS}
    assert {c["out_dim"] for c in GC.CASES} >= {GC.THIN_OUT - 1, GC.THIN_OUT, GC.THIN_OUT + 1}
    assert sorted(c["hidden"] for c in GC.CASES if not c["mask"]) == [4, 8, 12]  # the unmasked cases are small panels


@pytest.mark.parametrize("cid", GC.IDS)
def test_edge_case_keeps_the_relu_gate_out_of_the_comparison(cid):
    """tau = 32 x the float32 restatement's error on h_L.  Masked cases: every entry within tau of zero is masked, at most 0.1 % of the
    panel.  Unmasked cases: no entry within tau, and the case's seed is the first of its searched range with that property."""
    case = GC.BY_ID[cid]
    b = GC.build(cid)
    assert b["tau"] > 0 and GC.gate_is_clear(b)
    print("\n%s tau %.3e  smallest |h_L| %.3e  within tau %d of %d (%.4f %%)" % (cid, b["tau"], float(b["h64"].abs().min()), b["near"], b["h64"].numel(),
                                                                              100.0 * b["near"] / b["h64"].numel()))
    if b["mask"] is not None:
        assert b["near"] <= GC.MASKED_SHARE * b["h64"].numel()
        assert not bool(((b["h64"].abs() < b["tau"]) & (b["mask"] != 0)).any())
        assert set(b["mask"].unique().tolist()) <= {0.0, 2.0}
    else:
        assert case["searched"] == (1, case["seed"])
        assert b["near"] == 0 and float(b["h64"].abs().min()) >= b["tau"]
        assert not any(GC.seed_is_clear(case, s) for s in range(1, case["seed"]))


@pytest.mark.parametrize("cid", [c["id"] for c in GC.CASES if sum(GC.graph_sizes(c)[0]) <= GC.DENSE_REF_NODES])
def test_dense_restatement_agrees_with_the_index_add_one(cid):
    """Repeated edges add up and an explicit self loop is a diagonal entry of A, independently of `index_add_`: float64, 1e-12."""
    b = GC.build(cid)
    dense = GC.reference(b["model"], b["x"], b["ref_ei"], b["ref_ea"], b["mask"], b["d_out"], torch.float64, dense=True)
    for name, d, r in zip(GC.NAMES, dense, b["ref"]):
        assert d.shape == r.shape and _rel(d, r) <= 1e-12, (name, _rel(d, r))


def test_dense_restatement_by_hand():
    """Edge 0 -> 1 given twice (weights 3 and -1) and a self loop of weight 2 on node 1: A = [[0, 0], [2, 2]]."""
    conv = ggnn_ref.GatedGraphConv(2, 1, dense=True).double()
    with torch.no_grad():
        conv.weight[0] = torch.eye(2)
    x = torch.tensor([[1.0, 2.0], [5.0, 7.0]], dtype=torch.float64)
    h = conv(x, torch.tensor([[0, 1, 0], [1, 1, 1]]), torch.tensor([3.0, 2.0, -1.0], dtype=torch.float64))
    want1 = conv.rnn(2.0 * x[0:1] + 2.0 * x[1:2], x[1:2])
    assert torch.allclose(h[0:1], conv.rnn(torch.zeros(1, 2, dtype=torch.float64), x[0:1])) and torch.allclose(h[1:2], want1)
