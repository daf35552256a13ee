"""GPU tests of the HIP g-U-Net (csrc/k_unet.hip; scripts/Networks.py:125-449): the selection and the augment-and-filter kernels on
their own (exact), the trunk through the C ABI (`unet_forward_raw` / `unet_backward_raw` are the ctypes calls of drlgx_unet_forward /
drlgx_unet_backward) and through the modules against the plain-torch restatement tests/unet_ref.py in float64 on the CPU, the
trainers with directly constructed g-U-Net pairs, and FusedAdam beyond eight tensors.

Bound of the trunk comparisons, per tensor (the read-out and the 5 depth + 4 gradients), on e = max|delta| / max|ref|: at most 4 x
the error of the SAME restatement evaluated in float32 on the CPU at that shape, and never tighter than 2e-5 (the rule of
test_gpu_ggnn.py).  The selection is discrete, so every case first asserts on the float64 reference alone that at every level and
graph the k-th and the (k+1)-th score are at least 1e-3 x the level's largest |score| apart (fifty times the float32 floor), and the
kept sets are compared exactly.  Every case prints its ratios before it asserts."""
import ctypes as C
import math

import pytest
import torch

import unet_ref

pytestmark = pytest.mark.gpu

FLOOR, FACTOR, GAP = 2e-5, 4.0, 1e-3


def rel(a, ref):
    d, m = float((a.double() - ref).abs().max()), float(ref.abs().max())
    return d / m if m > 0 else (0.0 if d == 0 else math.inf)


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def offsets(sizes, dev=None):
    off = torch.tensor([0] + list(sizes)).cumsum(0).int()
    return off if dev is None else off.to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# the selection alone
# ---------------------------------------------------------------------------------------------------------------------
def rank_rule(scores, sizes, ratio):
    """The kept nodes by the rule itself, in plain Python: larger score first, equal scores to the lower index."""
    perm, off = [], 0
    for n in sizes:
        k = unet_ref.keep_count(n, ratio)
        order = sorted(range(n), key=lambda i: (-scores[off + i], i))
        perm += sorted(off + i for i in order[:k])
        off += n
    return perm


@pytest.mark.parametrize("ratio", [0.5, 0.8])
@pytest.mark.parametrize("kind", ["random", "ties", "equal"])
def test_selection_is_exact(kind, ratio):
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    sizes = [1, 2, 3, 64, 65, 257, 1100]  # across the wave (64), the chunk (256) and the LDS tile (1024)
    N, G = sum(sizes), len(sizes)
    gen = torch.Generator().manual_seed(11)
    if kind == "random":
        s = torch.tanh(torch.randn(N, generator=gen))
    elif kind == "equal":
        s = torch.full((N,), 0.25)
    else:  # few distinct values: exact ties across the k-th place of every graph
        s = torch.randint(0, 3, (N,), generator=gen).float() * 0.5 - 0.5
    want = rank_rule(s.tolist(), sizes, ratio)
    node_off = offsets(sizes, dev)
    pooled_off = torch.full((G + 1,), -7, dtype=torch.int32, device=dev)
    pooled_eoff = torch.full((G + 1,), -7, dtype=torch.int32, device=dev)
    perm = torch.full((N + 8,), -7, dtype=torch.int32, device=dev)
    inv = torch.full((N,), -7, dtype=torch.int32, device=dev)
    s_dev = s.to(dev)
    assert L.drlgx_unet_topk(None, N, G, vp(node_off), vp(s_dev), ratio, vp(pooled_off), vp(pooled_eoff), vp(perm), vp(inv)) == 0
    torch.cuda.synchronize()
    ks = [unet_ref.keep_count(n, ratio) for n in sizes]
    assert pooled_off.cpu().tolist() == offsets(ks).tolist()  # n_g <- ceil(ratio n_g)
    assert pooled_eoff.cpu().tolist() == offsets([k * (k - 1) for k in ks]).tolist()
    got = perm.cpu().tolist()
    assert got[:len(want)] == want and all(v == -7 for v in got[len(want):])  # nothing past the kept nodes
    inverse = [-1] * N
    for m, n in enumerate(want):
        inverse[n] = m
    assert inv.cpu().tolist() == inverse


# ---------------------------------------------------------------------------------------------------------------------
# augment and filter alone: small-integer weights, float32 is exact
# ---------------------------------------------------------------------------------------------------------------------
def star(n, inward, off=0):
    leaves, hub = torch.arange(1, n) + off, torch.full((n - 1,), off, dtype=torch.long)
    return torch.stack([leaves, hub]) if inward else torch.stack([hub, leaves])


def augment_case(kind, gen):
    """(sizes, edge_index grouped by graph, integer weights, kept nodes or None for 'the first ceil(n / 2) by a random score')"""
    if kind == "fan":
        return [3], torch.tensor([[0, 0], [1, 2]]), torch.tensor([2.0, 3.0]), torch.tensor([0, 1, 2])
    if kind in ("star_in", "star_out"):  # a row / a column of 70; (A + I)^2 is dense on the leaves for neither: the hub's row / column
        return [71], star(71, kind == "star_in"), torch.randint(1, 4, (70,), generator=gen).float(), None
    if kind == "star_both":  # both directions: the product is dense
        ei = torch.cat([star(71, True), star(71, False)], 1)
        return [71], ei, torch.randint(1, 4, (140,), generator=gen).float(), None
    if kind == "star_drop_hub":
        ei = torch.cat([star(71, True), star(71, False)], 1)
        return [71], ei, torch.randint(1, 4, (140,), generator=gen).float(), torch.arange(1, 37)
    if kind == "isolated":
        return [4], torch.tensor([[0, 1, 2], [1, 2, 0]]), torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0, 1, 3])
    if kind == "duplicates":  # 0 -> 1 twice (weights sum to 5), and an explicit self loop on 2 (sums with the added 1)
        return [3], torch.tensor([[0, 0, 1, 2], [1, 1, 2, 2]]), torch.tensor([2.0, 3.0, 1.0, 4.0]), torch.tensor([0, 1, 2])
    sizes, parts, ws, off = [5, 1, 11, 2], [], [], 0  # "batch"
    for k in sizes:
        if k > 1:
            src = torch.randint(0, k, (3 * k,), generator=gen)
            dst = (src + 1 + torch.randint(0, k - 1, (3 * k,), generator=gen)) % k
            parts.append(torch.stack([src, dst]) + off)
            ws.append(torch.randint(1, 4, (3 * k,), generator=gen).float())
        off += k
    return sizes, torch.cat(parts, 1), torch.cat(ws), None


@pytest.mark.parametrize("kind", ["fan", "star_in", "star_out", "star_both", "star_drop_hub", "isolated", "duplicates", "batch"])
def test_augment_and_filter_is_exact(kind):
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(17)
    sizes, ei, ew, perm = augment_case(kind, gen)
    N, E, G = sum(sizes), ei.shape[1], len(sizes)
    node_off = offsets(sizes)
    per = torch.bucketize(ei[0], node_off[1:].long(), right=True)
    edge_off = offsets(torch.bincount(per, minlength=G).tolist())
    if perm is None:
        perm, _ = unet_ref.select(torch.rand(N, generator=gen), sizes, 0.5)
        ks = [unet_ref.keep_count(n, 0.5) for n in sizes]
    else:
        ks = [int(perm.numel())]
    pooled_off, pooled_eoff = offsets(ks), offsets([k * (k - 1) for k in ks])
    cap = int(pooled_eoff[-1])
    out_ei = torch.full((2, cap + 4), -5, dtype=torch.int64, device=dev)[:, :cap].contiguous() if cap else torch.zeros(2, 0, dtype=torch.int64, device=dev)
    out_ew = torch.full((cap,), -5.0, device=dev)
    counts = torch.full((G,), -5, dtype=torch.int32, device=dev)
    d = [t.to(dev) for t in (ei, ew, node_off, edge_off, perm.int(), pooled_off, pooled_eoff)]  # (kept alive across the call)
    rc = L.drlgx_unet_augment_filter(None, N, E, vp(d[0]), vp(d[1]), G, vp(d[2]), vp(d[3]), max(sizes), vp(d[4]), vp(d[5]), vp(d[6]), cap, vp(out_ei),
                                     vp(out_ew), vp(counts))
    assert rc == 0
    torch.cuda.synchronize()
    want_ei, want_ew, want_counts = unet_ref.augment_filter(ei, ew.double(), sizes, perm, ks)
    assert counts.cpu().tolist() == want_counts
    oe, ow = out_ei.cpu(), out_ew.cpu()
    got = set()
    for g in range(G):
        a, n = int(pooled_eoff[g]), want_counts[g]
        rows = list(zip(oe[0, a:a + n].tolist(), oe[1, a:a + n].tolist(), ow[a:a + n].tolist()))
        assert rows == sorted(rows) and len(set(r[:2] for r in rows)) == n  # by (row, column), each once
        got |= set(rows)
        assert bool((oe[:, a + n:int(pooled_eoff[g + 1])] == -1).all())  # unused slots are marked
    assert got == set(zip(want_ei[0].tolist(), want_ei[1].tolist(), want_ew.tolist()))
    if kind == "fan":  # rows are sources: 0 -> 1, 0 -> 2 squared stays in row 0 (a transposed product would fill column 0)
        assert got == {(0, 1, 4.0), (0, 2, 6.0)}
    if kind == "duplicates":
        assert got == {(0, 1, 5.0 + 5.0), (1, 2, 1.0 + 5.0), (0, 2, 5.0)}


# ---------------------------------------------------------------------------------------------------------------------
# the trunk
# ---------------------------------------------------------------------------------------------------------------------
def random_edges(n, m, gen):
    src = torch.randint(0, n, (m,), generator=gen)
    dst = (src + 1 + torch.randint(0, n - 1, (m,), generator=gen)) % n
    return torch.stack([src, dst]), torch.rand(m, generator=gen) * 2.9 + 0.1


def batch_of(sizes, gen, per_node=3):
    parts, ws, off = [], [], 0
    for k in sizes:
        if k > 1:
            e, w = random_edges(k, per_node * k, gen)
            parts.append(e + off)
            ws.append(w)
        off += k
    return torch.cat(parts, 1), torch.cat(ws)


def wide_gemm_nodes():
    """The smallest node count whose N x 1000 . 1000 x 1000 product leaves the 64 x 64 kernels (the library's own dispatch rule), + 3."""
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    n = 1
    while L.drlgx_debug_gemm_tile_rows(n, 1000, 1, 0) == 64064:
        n += 1
        assert n < 100000
    return n + 3


def graph_case(kind, gen):
    """(x, edge_index, edge_attr, node counts per graph or None for one graph)"""
    sizes = None
    if kind == "single":
        n, ei, ea = 1, torch.zeros(2, 0, dtype=torch.long), torch.zeros(0)
    elif kind == "two":
        n, ei, ea = 2, torch.tensor([[0], [1]]), torch.tensor([1.3])
    elif kind == "fan":
        n, ei, ea = 3, torch.tensor([[0, 0], [1, 2]]), torch.tensor([0.7, 2.3])
    elif kind == "isolated":
        n = 7
        ei, ea = random_edges(6, 13, gen)
    elif kind in ("star_in", "star_out"):
        n, ei, ea = 71, star(71, kind == "star_in"), torch.rand(70, generator=gen) * 0.5 + 0.05
    elif kind == "batch":
        sizes = [5, 1, 11, 2]
        n = sum(sizes)
        ei, ea = batch_of(sizes, gen)
    elif kind == "n130":
        n = 130
        ei, ea = random_edges(n, 4 * n, gen)
    else:  # "wide": two graphs that together pass the dispatcher's switch (few graphs: every graph adds a k-th place that must be clear)
        total = wide_gemm_nodes()
        sizes = [total // 2, total - total // 2]
        n = total
        ei, ea = batch_of(sizes, gen, 4)
    x = torch.randn(n, 5, generator=gen)
    x[:, 4] = torch.randint(-1, 2, (n,), generator=gen).float()
    return x, ei, ea, sizes


def segments(sizes, ei, dev):
    """(n_graphs, node_off, edge_off, largest node count) of a batch whose edges are grouped by graph."""
    node_off = offsets(sizes)
    per = torch.bucketize(ei[0], node_off[1:].long(), right=True)
    edge_off = offsets(torch.bincount(per, minlength=len(sizes)).tolist())
    return (len(sizes), node_off.to(dev), edge_off.to(dev), max(sizes))


def reference(model, x, ei, ea, mask, d_out, sizes, dtype):
    """out and the gradients of sum(out * d_out) from the restatement at `dtype` as float64 tensors, and its levels."""
    m = unet_ref.RefGraphUNet(x.shape[1], model.fully_con1.in_features, model.depth, model.ratio, model.fully_con1.out_features).to(dtype)
    m.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()})
    out = m(x.to(dtype), ei, ea.to(dtype), None if mask is None else mask.to(dtype), sizes)
    (out * d_out.to(dtype)).sum().backward()
    return [out.detach().double()] + [p.grad.double() for p in m.trunk_parameters()], m.levels


def assert_gaps(levels):
    """The precondition of a comparison across a discrete selection, on the float64 reference alone."""
    for l, lv in enumerate(levels):
        assert min(lv["gaps"]) >= GAP * lv["max_abs"], ("level %d: k-th / (k+1)-th scores %.3e apart, largest |score| %.3e" % (l + 1, min(lv["gaps"]), lv["max_abs"]))


def hip_run(model, x, ei, ea, mask, d_out, dev, segs=None):
    from drl_graph_exploration_amd.networks import unet_backward_raw, unet_forward_raw, unet_kept_nodes
    params = tuple(p.detach().to(dev) for p in model.trunk_parameters())
    md = None if mask is None else mask.to(dev)
    out, saved = unet_forward_raw(x.to(dev), ei.to(dev), ea.to(dev), params, model.depth, model.ratio, md, segs)
    grads = tuple(torch.full_like(p, float("nan")) for p in params)  # (written, not accumulated)
    unet_backward_raw(saved, d_out.to(dev), grads)
    kept = [unet_kept_nodes(saved, l).cpu().long() for l in range(1, model.depth + 1)]
    return [out.cpu()] + [g.cpu() for g in grads], kept


def names_of(model):
    return ["out"] + ["d_" + k for k, _ in model.named_parameters()]


CASES = [
    # kind, hidden, depth, out_dim, mask, ratio, seed
    ("single", 1000, 3, 1, False, 0.5, 1),
    ("two", 1000, 3, 1, True, 0.5, 1),
    ("fan", 1000, 3, 1, True, 0.5, 1),
    ("isolated", 1000, 3, 100, True, 0.5, 1),
    ("isolated", 8, 1, 1, True, 0.8, 1),
    ("star_in", 1000, 3, 1, False, 0.5, 9),
    ("star_out", 1000, 2, 100, False, 0.5, 1),
    ("batch", 1000, 3, 1, True, 0.5, 1),
    ("batch", 8, 2, 100, False, 0.5, 1),
    ("n130", 1000, 3, 1, True, 0.5, 38),
    ("n130", 8, 2, 3, False, 0.8, 1),
    ("wide", 1000, 1, 1, True, 0.8, 2),
]


def build_case(kind, hidden, depth, out_dim, with_mask, ratio, seed):
    gen = torch.Generator().manual_seed(1000 * seed + 7 * len(kind) + hidden + depth + out_dim)
    torch.manual_seed(100 * seed + hidden + depth + out_dim)
    model = unet_ref.RefGraphUNet(5, hidden, depth, ratio, out_dim)  # random weights: the modules' own init
    with torch.no_grad():
        # GCNConv's biases start at zero: give them values that matter.  Every gate multiplies the activations by |s| ~ 0.1, so a
        # down conv's bias is drawn at its level's scale - a larger one would be all a deep level's scores see, and no seed separates them
        for k, p in model.named_parameters():
            if k.endswith("bias") and "conv" in k:
                scale = 0.05 * 0.1 ** int(k.split(".")[1]) if k.startswith("down") else 0.05
                p.uniform_(-scale, scale)
    x, ei, ea, sizes = graph_case(kind, gen)
    N = x.shape[0]
    mask = (torch.rand(N, hidden, generator=gen) >= 0.5).float() * 2.0 if with_mask else None
    d_out = torch.randn(N, out_dim, generator=gen)
    return model, x, ei, ea, sizes, mask, d_out


@pytest.mark.parametrize("kind,hidden,depth,out_dim,with_mask,ratio,seed", CASES,
                         ids=["%s-h%d-d%d-o%d-%s-r%g" % (c[0], c[1], c[2], c[3], "mask" if c[4] else "nomask", c[5]) for c in CASES])
def test_trunk_matches_the_float64_restatement(kind, hidden, depth, out_dim, with_mask, ratio, seed):
    dev = torch.device("cuda", 0)
    model, x, ei, ea, sizes, mask, d_out = build_case(kind, hidden, depth, out_dim, with_mask, ratio, seed)
    N = x.shape[0]
    ref, levels = reference(model, x, ei, ea, mask, d_out, sizes, torch.float64)
    assert_gaps(levels)
    ref32, _ = reference(model, x, ei, ea, mask, d_out, sizes, torch.float32)
    segs = None if sizes is None else segments(sizes, ei, dev)
    got, kept = hip_run(model, x, ei, ea, mask, d_out, dev, segs)
    again, _ = hip_run(model, x, ei, ea, mask, d_out, dev, segs)
    for l, lv in enumerate(levels):  # the kept sets, exactly
        assert kept[l].tolist() == lv["perm"].tolist(), "level %d" % (l + 1)
    names, report = names_of(model), []
    for name, g, r, r32 in zip(names, got, ref, ref32):
        assert g.shape == r.shape, name
        e, e32 = rel(g, r), rel(r32, r)
        report.append((name, e, e32, max(FACTOR * e32, FLOOR)))
    print("\n%s N=%d E=%d hidden=%d depth=%d out=%d mask=%s ratio=%g" % (kind, N, ei.shape[1], hidden, depth, out_dim, with_mask, ratio))
    for name, e, e32, bound in report:
        print("  %-22s hip %.3e  fp32 cpu %.3e  ratio %s  bound %.3e" % (name, e, e32, "%.2f" % (e / e32) if e32 > 0 else "-", bound))
    for name, e, e32, bound in report:
        assert e <= bound, (name, e, e32)
    for name, a, b in zip(names, got, again):  # deterministic reductions: two runs are bit-equal
        assert torch.equal(a, b), name
    if sizes is None and N > 1:  # one graph given as one segment: the one-launch CSR build, the same bits
        seg, _ = hip_run(model, x, ei, ea, mask, d_out, dev, segments([N], ei, dev))
        for name, a, b in zip(names, got, seg):
            assert torch.equal(a, b), name


def test_invalid_arguments_and_a_small_workspace_are_refused():
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    buf = torch.zeros(1 << 10, device=dev)  # (zeros serve as x and as every parameter of the one valid call)
    nbytes = L.drlgx_unet_workspace_bytes(2, 0, 0, 2, 8, 2, 0.5, 1)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    out = torch.full((2,), 5.0, device=dev)
    p, pw, po = C.c_void_p(buf.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr())

    def fwd(n=2, in_dim=5, hidden=8, depth=2, ratio=0.5, x=p, wsb=nbytes, max_nodes=2, params=14):
        arr = (C.c_void_p * 24)(*([buf.data_ptr()] * params + [None] * (24 - params)))
        return L.drlgx_unet_forward(None, n, 0, in_dim, hidden, depth, ratio, 1, x, None, None, arr, None, po, pw, wsb, 0, None, None, max_nodes)

    assert nbytes > 0
    # a workspace size argument that is too small: the code, and nothing written (neither the output nor the workspace)
    assert fwd(wsb=nbytes - 512) == -3 and fwd(wsb=0) == -3
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((ws == 0).all())
    assert fwd(max_nodes=1) == -3  # the graph has more nodes than the caller's bound
    assert fwd() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())  # zero weights, bf = 0
    assert fwd(in_dim=9) == -1 and fwd(hidden=10) == -1 and fwd(depth=0) == -1 and fwd(depth=5) == -1 and fwd(x=None) == -1
    assert fwd(ratio=0.0) == -1 and fwd(ratio=1.5) == -1 and fwd(params=13) == -1
    assert L.drlgx_unet_workspace_bytes(2, 0, 0, 2, 8, 0, 0.5, 1) == 0 and L.drlgx_unet_workspace_bytes(2, 0, 0, 2, 8, 5, 0.5, 1) == 0
    assert L.drlgx_unet_workspace_bytes(5000, 0, 0, 5000, 8, 1, 0.5, 1) == 0  # a graph beyond the augment's dense rows
    assert L.drlgx_unet_topk(None, 2, 1, None, p, 0.5, p, None, p, None) == -1
    assert L.drlgx_unet_augment_filter(None, 2, 0, None, None, 1, p, p, 5000, p, p, p, 0, None, None, None) == -3


def module_batch():
    gen = torch.Generator().manual_seed(5)
    x, ei, ea, sizes = graph_case("batch", gen)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return x, ei, ea, sizes, batch


def module_reference(model, x, ei, ea, mask, d_out, sizes, dtype):
    m = unet_ref.RefGraphUNet(5, 1000, model.depth, model.pool_ratios[0], model.fully_con1.out_features).to(dtype)
    m.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()})
    out = m(x.to(dtype), ei, ea.to(dtype), None if mask is None else mask.to(dtype), sizes)
    if d_out is not None:
        (out * d_out.to(dtype)).sum().backward()
    return m, out.detach()


def test_graph_unet_module_matches_the_restatement_through_autograd():
    from drl_graph_exploration_amd.networks import GraphData, GraphUNet
    dev = torch.device("cuda", 0)
    x, ei, ea, sizes, batch = module_batch()
    torch.manual_seed(3)
    model = GraphUNet(5, 1000, 1000, 3)
    d_out = torch.randn(x.shape[0], 1, generator=torch.Generator().manual_seed(8))
    m64, out64 = module_reference(model, x, ei, ea, None, d_out, sizes, torch.float64)
    assert_gaps(m64.levels)
    m32, out32 = module_reference(model, x, ei, ea, None, d_out, sizes, torch.float32)
    model.to(dev)
    q = model(GraphData(x.to(dev), ei.to(dev), ea.to(dev), batch.to(dev)), 0.0, batch=batch.to(dev))  # boundaries from the batch vector
    assert q.shape == (x.shape[0], 1)
    assert rel(q.detach().cpu(), out64.double()) <= max(FACTOR * rel(out32.double(), out64.double()), FLOOR)
    (q * d_out.to(dev)).sum().backward()
    for (name, p), r, r32 in zip(model.named_parameters(), m64.parameters(), m32.parameters()):
        assert p.grad is not None, name
        e, e32 = rel(p.grad.cpu(), r.grad.double()), rel(r32.grad.double(), r.grad.double())
        print("  %-22s hip %.3e  fp32 cpu %.3e" % (name, e, e32))
        assert e <= max(FACTOR * e32, FLOOR), name


@pytest.mark.parametrize("with_segments", [False, True])
def test_policy_and_value_heads_match_the_restatement(monkeypatch, with_segments):
    """PolicyGraphUNet / ValueGraphUNet with the dropout mask frozen for the comparison (F.dropout with p = 0.5 is always on), with and
    without the batch's graph boundaries; the heads work over the ORIGINAL batch vector."""
    import drl_graph_exploration_amd.networks as NW
    dev = torch.device("cuda", 0)
    x, ei, ea, sizes, batch = module_batch()
    N, G = x.shape[0], len(sizes)
    sel = x[:, 4] > 0
    for g in range(G):
        sel[int((batch == g).nonzero()[0])] = True  # every graph has a candidate
    fixed = (torch.rand(N, 1000, generator=torch.Generator().manual_seed(21)) >= 0.5).float() * 2.0
    fixed_dev = fixed.to(dev)
    monkeypatch.setattr(NW, "_dropout_mask", lambda n, hidden, p, device: fixed_dev if p > 0 else None)
    torch.manual_seed(11)  # (a seed whose float64 reference keeps every k-th place clear, see assert_gaps)
    pol, val = NW.PolicyGraphUNet(5, 1000, 1000, 3), NW.ValueGraphUNet(5, 1000, 1000, 3)

    def heads(dtype):
        out = []
        for model, head in ((pol, lambda q: unet_ref.policy_head(q, sel, batch, G)), (val, lambda h: unet_ref.value_head(h, batch, G))):
            m, o = module_reference(model, x, ei, ea, fixed, None, sizes, dtype)
            if dtype == torch.float64:
                assert_gaps(m.levels)
            out.append(head(o).double())
        return out

    ref, ref32 = heads(torch.float64), heads(torch.float32)
    pol.to(dev), val.to(dev)
    seg = segments(sizes, ei, dev) if with_segments else (None, None, None, None)
    data = NW.GraphData(x.to(dev), ei.to(dev), ea.to(dev), batch.to(dev), seg[1], seg[2], int(torch.bincount(batch[ei[0]]).max()) if with_segments else None)
    probs, values = pol(data, sel.to(dev), batch=batch.to(dev)), val(data, sel.to(dev), batch=batch.to(dev))
    assert probs.shape == (int(sel.sum()),) and values.shape == (G,)
    for got, r, r32 in ((probs, ref[0], ref32[0]), (values, ref[1], ref32[1])):
        assert rel(got.detach().cpu(), r) <= max(FACTOR * rel(r32, r), FLOOR)
    (probs.log().sum() + values.sum()).backward()
    for p in list(pol.parameters()) + list(val.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())


# ---------------------------------------------------------------------------------------------------------------------
# trainers and optimiser
# ---------------------------------------------------------------------------------------------------------------------
def test_deepq_runs_with_a_graph_unet_pair(tmp_path):
    """DeepQ with directly constructed g-U-Nets takes the generic (framework) update path with FusedAdam: nineteen tensors."""
    from drl_graph_exploration_amd.networks import GraphUNet
    from drl_graph_exploration_amd.policy import DeepQ
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dq = DeepQ("DQN_g-U-Net/", "g-U-Net", data_root=str(tmp_path))
    dq.OBSERVE, dq.epoch, dq.BATCH = 8, 16, 8
    pol, tgt = GraphUNet(5, 1000, 1000, 3).to(dev), GraphUNet(5, 1000, 1000, 3).to(dev)
    tgt.load_state_dict(pol.state_dict())
    before = [p.detach().clone() for p in pol.parameters()]
    dq.running(pol, tgt, test=True, n_envs=4)
    assert dq.step_t == 16 and len(dq.buffer) == 16
    assert dq.temp_loss > 0 and math.isfinite(dq.temp_loss)
    assert all(bool(torch.isfinite(p).all()) for p in pol.parameters())
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, pol.parameters()))
    sd = torch.load(tmp_path / "training_object_data" / "DQN_g-U-Net" / "Model_Policy.pt", map_location="cpu")
    assert list(sd.keys()) == list(unet_ref.RefGraphUNet(5, 8, 3, 0.5, 1).state_dict().keys())


def test_a2c_runs_with_a_graph_unet_pair(tmp_path):
    import numpy as np
    from drl_graph_exploration_amd.networks import PolicyGraphUNet, ValueGraphUNet
    from drl_graph_exploration_amd.policy import A2C
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    np.random.seed(0)
    a2c = A2C("A2C_g-U-Net/", data_root=str(tmp_path))
    a2c.nstep, a2c.epoch, a2c.graphs_per_pass = 2, 8, 5  # 2 vector steps of 4 envs: one update
    actor, critic = PolicyGraphUNet(5, 1000, 1000, 3).to(dev), ValueGraphUNet(5, 1000, 1000, 3).to(dev)
    wa, wc = [p.detach().clone() for p in actor.parameters()], [p.detach().clone() for p in critic.parameters()]
    a2c.running(actor, critic, test=True, n_envs=4)
    assert a2c.step_t == 8
    assert math.isfinite(a2c.temp_loss) and a2c.temp_loss != 0
    for before, model in ((wa, actor), (wc, critic)):
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
        assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    for f in ("Model_Policy.pt", "Model_Value.pt"):
        assert (tmp_path / "training_object_data" / "A2C_g-U-Net" / f).exists()


def test_fused_adam_steps_nineteen_tensors_and_six_as_before():
    from drl_graph_exploration_amd import _lib
    from drl_graph_exploration_amd.networks import GraphUNet
    from drl_graph_exploration_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    torch.manual_seed(6)
    lr, clamp = 1e-3, 0.5
    model = GraphUNet(5, 64, 64, 3).to(dev)
    twin = GraphUNet(5, 64, 64, 3).to(dev)
    twin.load_state_dict(model.state_dict())
    assert len(list(model.parameters())) == 19
    opt, ref = FusedAdam(model.parameters(), lr=lr, grad_clamp=clamp), torch.optim.Adam(twin.parameters(), lr=lr)
    gen = torch.Generator().manual_seed(9)
    for step in range(3):
        opt.zero_grad()
        for p, q in zip(model.parameters(), twin.parameters()):
            g = (torch.randn(p.shape, generator=gen) * 0.7).to(dev)  # some elements beyond the clamp
            p.grad.copy_(g)
            q.grad = g.clamp(-clamp, clamp)
        opt.step()
        ref.step()
        for (k, a), b in zip(model.state_dict().items(), twin.state_dict().values()):
            # one Adam step moves a parameter by at most ~lr: the two must agree to a small fraction of that
            assert float((a - b).abs().max()) < 2e-2 * lr * (step + 1), (step, k)
    assert opt.step_count == 3
    # six tensors: the same single launch as before the grouping - bit-equal to drlgx_adam_step_scaled called directly
    torch.manual_seed(7)
    ps = [torch.randn(s, device=dev) for s in ((5, 40), (40,), (40, 40), (40,), (1, 40), (1,))]
    qs = [p.clone() for p in ps]
    gs = [torch.randn(p.shape, device=dev) for p in ps]
    opt6 = FusedAdam(ps, lr=lr, grad_clamp=clamp)
    m, v = [torch.zeros_like(q) for q in qs], [torch.zeros_like(q) for q in qs]
    arr = lambda ts: (C.c_void_p * 6)(*[t.data_ptr() for t in ts])  # noqa: E731
    sizes = (C.c_int64 * 6)(*[q.numel() for q in qs])
    for step in range(1, 3):
        for g_view, g in zip(opt6.grads(), gs):
            g_view.copy_(g * step)
        opt6.step()
        gq = [g * step for g in gs]
        _lib.check(_lib.lib().drlgx_adam_step_scaled(C.c_void_p(_lib.stream_ptr(dev)), 6, arr(qs), arr(gq), arr(m), arr(v), sizes, lr, 0.9, 0.999, 1e-8,
                                                     step, clamp, 1.0))
    torch.cuda.synchronize()
    for a, b in zip(ps, qs):
        assert torch.equal(a, b)
