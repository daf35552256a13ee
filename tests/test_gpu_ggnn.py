"""GPU tests of the HIP GG-NN trunk (csrc/k_ggnn.hip; scripts/Networks.py:73-122) through the C ABI (`ggnn_forward_raw` /
`ggnn_backward_raw` are the ctypes calls of drlgx_ggnn_forward / drlgx_ggnn_backward) and through the modules, against the
plain-torch restatement tests/ggnn_ref.py evaluated in float64 on the CPU.

Bound, per tensor (the read-out and the seven gradients), on e = max|delta| / max|ref|: at most 4 x the error of the SAME
restatement evaluated in float32 on the CPU at that shape (the factor covers the other summation order of split-K and the matrix
cores), and never tighter than 2e-5 (the GCN trunk's figure, so that a lucky float32 run cannot make the bound vacuous).
Every case prints its ratios before it asserts."""
import math

import pytest
import torch

import ggnn_ref

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 2e-5, 4.0
NAMES = ("out", "d_weight", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh", "dWf", "dbf")


def rel(a, ref):
    d, m = float((a.double() - ref).abs().max()), float(ref.abs().max())
    return d / m if m > 0 else (0.0 if d == 0 else math.inf)


def random_edges(n, m, gen):
    """m directed edges without self loops, asymmetric (the reverse of an edge is not added), positive weights."""
    src = torch.randint(0, n, (m,), generator=gen)
    dst = (src + 1 + torch.randint(0, n - 1, (m,), generator=gen)) % n
    return torch.stack([src, dst]), torch.rand(m, generator=gen) * 2.9 + 0.1


def graph_case(kind, gen):
    """(x, edge_index, edge_attr, node counts per graph or None)"""
    sizes = None
    if kind == "single":  # N = 1, E = 0
        n, ei, ea = 1, torch.zeros(2, 0, dtype=torch.long), torch.zeros(0)
    elif kind == "fan":  # only 0 -> 1 and 0 -> 2: a swapped aggregation direction shows
        n, ei, ea = 3, torch.tensor([[0, 0], [1, 2]]), torch.tensor([0.7, 2.3])
    elif kind == "isolated":  # 7 nodes (no multiple of kAggNodes), node 6 has no edge
        n = 7
        ei, ea = random_edges(6, 13, gen)
    elif kind in ("star_in", "star_out"):  # 70 leaves and a hub: a by-destination / by-source row longer than kAggStage
        n = 71
        leaves, hub = torch.arange(1, 71), torch.zeros(70, dtype=torch.long)
        ei = torch.stack([leaves, hub]) if kind == "star_in" else torch.stack([hub, leaves])
        ea = torch.rand(70, generator=gen) * 0.5 + 0.05
    elif kind == "batch":  # three graphs of 5, 1 and 11 nodes
        sizes, parts, ws, off = [5, 1, 11], [], [], 0
        for k in sizes:
            if k > 1:
                e, w = random_edges(k, 3 * k, gen)
                parts.append(e + off)
                ws.append(w)
            off += k
        n, ei, ea = off, torch.cat(parts, 1), torch.cat(ws)
    else:  # ("nodes", N): E ~ 4 N
        n = kind[1]
        ei, ea = random_edges(n, 4 * n, gen)
    x = torch.randn(n, 5, generator=gen)
    x[:, 4] = torch.randint(-1, 2, (n,), generator=gen).float()
    return x, ei, ea, sizes


def segments(sizes, ei, dev):
    """(n_graphs, node_off, edge_off, max edges of a graph) of a batch whose edges are grouped by graph."""
    node_off = torch.tensor([0] + sizes).cumsum(0)
    per = torch.bucketize(ei[0], node_off[1:], right=True)
    counts = torch.bincount(per, minlength=len(sizes))
    edge_off = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    return (len(sizes), node_off.int().to(dev), edge_off.int().to(dev), int(counts.max()))


def wide_gemm_nodes():
    """The smallest node count whose N x 3000 gate product leaves the 64 x 64 kernels (asked of the library's own dispatch rule), + 3."""
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    n = 1
    while L.drlgx_debug_gemm_tile_rows(n, 3000, 1, 0) == 64064:
        n += 1
        assert n < 100000
    return n + 3


def reference(model, x, ei, ea, mask, d_out, dtype):
    """out and the seven gradients of sum(out * d_out) from the restatement at `dtype`, as float64 tensors."""
    m = ggnn_ref.RefGGNN(model.gconv1.out_channels, model.gconv1.num_layers, model.fully_con1.out_features).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in model.state_dict().items()})
    out = m(x.to(dtype), ei, ea.to(dtype), None if mask is None else mask.to(dtype))
    (out * d_out.to(dtype)).sum().backward()
    return [out.detach().double()] + [p.grad.double() for p in m.trunk_parameters()]


def hip_run(model, x, ei, ea, mask, d_out, dev, segs=None):
    from drl_graph_exploration_amd.networks import ggnn_backward_raw, ggnn_forward_raw
    params = tuple(p.detach().to(dev) for p in model.trunk_parameters())
    xd, eid, ead = x.to(dev), ei.to(dev), ea.to(dev)
    md = None if mask is None else mask.to(dev)
    out, saved = ggnn_forward_raw(xd, eid, ead, params, md, segs)
    grads = tuple(torch.full_like(p, float("nan")) for p in params)  # (written, not accumulated)
    ggnn_backward_raw(saved, d_out.to(dev), grads)
    return [out.cpu()] + [g.cpu() for g in grads]


CASES = [
    # kind, hidden, layers, out_dim, mask
    ("single", 1000, 3, 1, False),
    ("fan", 1000, 3, 1, True),
    ("isolated", 1000, 3, 100, True),
    ("isolated", 1000, 1, 1, True),
    ("star_in", 1000, 3, 1, False),
    ("star_out", 1000, 3, 100, False),
    ("batch", 1000, 3, 1, True),
    ("batch", 8, 2, 100, False),
    ("isolated", 8, 2, 3, True),
    ("wide", 1000, 3, 1, True),
]


@pytest.mark.parametrize("kind,hidden,layers,out_dim,with_mask", CASES, ids=["%s-h%d-L%d-o%d-%s" % (c[0], c[1], c[2], c[3], "mask" if c[4] else "nomask")
                                                                              for c in CASES])
def test_trunk_matches_the_float64_restatement(kind, hidden, layers, out_dim, with_mask):
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1234 + 7 * len(kind) + hidden + layers + out_dim)
    torch.manual_seed(99 + hidden + layers + out_dim)
    model = ggnn_ref.RefGGNN(hidden, layers, out_dim)  # random weights: the modules' own init
    x, ei, ea, sizes = graph_case(("nodes", wide_gemm_nodes()) if kind == "wide" else kind, gen)
    N = x.shape[0]
    mask = (torch.rand(N, hidden, generator=gen) >= 0.5).float() * 2.0 if with_mask else None
    d_out = torch.randn(N, out_dim, generator=gen)
    ref = reference(model, x, ei, ea, mask, d_out, torch.float64)
    ref32 = reference(model, x, ei, ea, mask, d_out, torch.float32)
    got = hip_run(model, x, ei, ea, mask, d_out, dev)
    again = hip_run(model, x, ei, ea, mask, d_out, dev)
    report = []
    for name, g, r, r32 in zip(NAMES, got, ref, ref32):
        assert g.shape == r.shape, name
        e, e32 = rel(g, r), rel(r32, r)
        report.append((name, e, e32, max(FACTOR * e32, FLOOR)))
    print("\n%s N=%d E=%d hidden=%d layers=%d out=%d mask=%s" % (kind, N, ei.shape[1], hidden, layers, out_dim, with_mask))
    for name, e, e32, bound in report:
        print("  %-9s hip %.3e  fp32 cpu %.3e  ratio %s  bound %.3e" % (name, e, e32, "%.2f" % (e / e32) if e32 > 0 else "-", bound))
    for name, e, e32, bound in report:
        assert e <= bound, (name, e, e32)
    for name, a, b in zip(NAMES, got, again):  # deterministic reductions: two runs are bit-equal
        assert torch.equal(a, b), name
    assert bool((got[1][0, 5:] == 0).all())  # rows in_dim.. of d_weight[0]: h_0's padding
    if sizes is not None:  # the batch's graph boundaries select the one-launch CSR build: the same bits
        seg = hip_run(model, x, ei, ea, mask, d_out, dev, segments(sizes, ei, dev))
        for name, a, b in zip(NAMES, got, seg):
            assert torch.equal(a, b), name


def test_invalid_arguments_are_refused():
    import ctypes as C
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    buf = torch.zeros(1 << 10, device=dev)  # (zeros serve as x and as every parameter of the one valid call)
    ws = torch.empty(L.drlgx_ggnn_workspace_bytes(2, 0, 8, 2, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(2, device=dev)
    p, pw, po = C.c_void_p(buf.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr())

    def fwd(n=2, e=0, in_dim=5, hidden=8, layers=2, out_dim=1, x=p):
        return L.drlgx_ggnn_forward(None, n, e, in_dim, hidden, layers, out_dim, x, None, None, p, p, p, p, p, p, p, None, po, pw, 0, None, None, 0)

    assert ws.numel() > 0 and fwd() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())  # relu(h) = 0 from zero weights, bf = 0
    assert fwd(in_dim=9, hidden=16) == -1 and fwd(in_dim=5, hidden=4) == -1 and fwd(hidden=10) == -1 and fwd(layers=0) == -1 and fwd(x=None) == -1
    assert L.drlgx_ggnn_workspace_bytes(2, 0, 8, 0, 1) == 0


def module_batch(dev):
    gen = torch.Generator().manual_seed(5)
    x, ei, ea, sizes = graph_case("batch", gen)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return x, ei, ea, sizes, batch


def test_ggnn_module_matches_the_restatement():
    from drl_graph_exploration_amd.networks import GGNN, GraphData
    dev = torch.device("cuda", 0)
    x, ei, ea, sizes, batch = module_batch(dev)
    torch.manual_seed(3)
    model = GGNN()
    d_out = torch.randn(x.shape[0], 1, generator=torch.Generator().manual_seed(8))
    ref = reference(model, x, ei, ea, None, d_out, torch.float64)
    ref32 = reference(model, x, ei, ea, None, d_out, torch.float32)
    model.to(dev)
    q = model(GraphData(x.to(dev), ei.to(dev), ea.to(dev), batch.to(dev)), 0.0, batch=batch.to(dev))
    assert q.shape == (x.shape[0], 1)
    assert rel(q.detach().cpu(), ref[0]) <= max(FACTOR * rel(ref32[0], ref[0]), FLOOR)
    # autograd through the module = drlgx_ggnn_backward on the same inputs, bit for bit
    (q * d_out.to(dev)).sum().backward()
    raw = hip_run(model, x, ei, ea, None, d_out, dev)
    for name, p, g in zip(NAMES[1:], model.trunk_parameters(), raw[1:]):
        assert p.grad is not None and torch.equal(p.grad.cpu(), g), name
    for name, p, r, r32 in zip(NAMES[1:], model.trunk_parameters(), ref[1:], ref32[1:]):
        assert rel(p.grad.cpu(), r) <= max(FACTOR * rel(r32, r), FLOOR), name


@pytest.mark.parametrize("with_segments", [False, True])
def test_policy_and_value_heads_match_the_restatement(monkeypatch, with_segments):
    """PolicyGGNN / ValueGGNN with the dropout mask frozen for the comparison (F.dropout with p = 0.5 is always on), with and
    without the batch's graph boundaries (HIP segment kernels / tensor-op heads)."""
    import drl_graph_exploration_amd.networks as NW
    dev = torch.device("cuda", 0)
    x, ei, ea, sizes, batch = module_batch(dev)
    N, G = x.shape[0], len(sizes)
    sel = x[:, 4] > 0
    for g in range(G):
        sel[int((batch == g).nonzero()[0])] = True  # every graph has a candidate
    fixed = (torch.rand(N, 1000, generator=torch.Generator().manual_seed(21)) >= 0.5).float() * 2.0
    fixed_dev = fixed.to(dev)
    monkeypatch.setattr(NW, "_dropout_mask", lambda n, hidden, p, device: fixed_dev if p > 0 else None)
    torch.manual_seed(4)
    pol, val = NW.PolicyGGNN(), NW.ValueGGNN()

    def heads(dtype):
        out = []
        for model, head in ((pol, lambda q: ggnn_ref.policy_head(q, sel, batch, G)), (val, lambda h: ggnn_ref.value_head(h, batch, G))):
            m = ggnn_ref.RefGGNN(1000, 3, model.fully_con1.out_features).to(dtype)
            m.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()})
            with torch.no_grad():
                out.append(head(m(x.to(dtype), ei, ea.to(dtype), fixed.to(dtype))).double())
        return out

    ref, ref32 = heads(torch.float64), heads(torch.float32)
    pol.to(dev), val.to(dev)
    seg = segments(sizes, ei, dev) if with_segments else (None, None, None, None)
    data = NW.GraphData(x.to(dev), ei.to(dev), ea.to(dev), batch.to(dev), seg[1], seg[2], seg[3])
    probs, values = pol(data, sel.to(dev), batch=batch.to(dev)), val(data, sel.to(dev), batch=batch.to(dev))
    assert probs.shape == (int(sel.sum()),) and values.shape == (G,)
    for got, r, r32 in ((probs, ref[0], ref32[0]), (values, ref[1], ref32[1])):
        assert rel(got.detach().cpu(), r) <= max(FACTOR * rel(r32, r), FLOOR)
    (probs.log().sum() + values.sum()).backward()
    for p in list(pol.parameters()) + list(val.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())


def test_deepq_runs_with_the_ggnn_pair(tmp_path):
    """DeepQ with GG-NN takes the generic (framework) update path with FusedAdam: seven tensors."""
    from drl_graph_exploration_amd.policy import DeepQ
    from drl_graph_exploration_amd.train import make_models
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dq = DeepQ("DQN_GG-NN/", "GG-NN", data_root=str(tmp_path))
    dq.OBSERVE, dq.epoch, dq.BATCH = 8, 16, 8
    pol, tgt = make_models("DQN", "GG-NN", dev)
    tgt.load_state_dict(pol.state_dict())
    before = [p.detach().clone() for p in pol.parameters()]
    dq.running(pol, tgt, test=True, n_envs=4)
    assert dq.step_t == 16 and len(dq.buffer) == 16
    assert dq.temp_loss > 0 and math.isfinite(dq.temp_loss)
    assert all(bool(torch.isfinite(p).all()) for p in pol.parameters())
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, pol.parameters()))
    sd = torch.load(tmp_path / "training_object_data" / "DQN_GG-NN" / "Model_Policy.pt", map_location="cpu")
    assert list(sd.keys()) == list(ggnn_ref.RefGGNN(8, 1, 1).state_dict().keys())


def test_a2c_runs_with_the_ggnn_pair(tmp_path):
    import numpy as np
    from drl_graph_exploration_amd.policy import A2C
    from drl_graph_exploration_amd.train import make_models
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    np.random.seed(0)
    a2c = A2C("A2C_GG-NN/", data_root=str(tmp_path))
    a2c.nstep, a2c.epoch, a2c.graphs_per_pass = 2, 8, 5  # 2 vector steps of 4 envs: one update
    actor, critic = make_models("A2C", "GG-NN", dev)
    wa, wc = [p.detach().clone() for p in actor.parameters()], [p.detach().clone() for p in critic.parameters()]
    a2c.running(actor, critic, test=True, n_envs=4)
    assert a2c.step_t == 8
    assert math.isfinite(a2c.temp_loss) and a2c.temp_loss != 0
    for before, model in ((wa, actor), (wc, critic)):
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
        assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    for f in ("Model_Policy.pt", "Model_Value.pt"):
        assert (tmp_path / "training_object_data" / "A2C_GG-NN" / f).exists()
