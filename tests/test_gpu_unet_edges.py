"""GPU tests of the g-U-Net pooling kernels (csrc/k_unet.hip) where their row passes and bit masks wrap; the cases, what each reaches and
the CPU checks of both are tests/unet_cases.py and tests/test_unet_cpu.py.

Augment-and-filter through drlgx_unet_augment_filter, exact (small-integer weights): k_unet_augment keeps T rows of a graph in flight
and walks the kept rows in passes of T, carrying the output position; T falls below the node count from 126 nodes and is 3 at the 4 096
cap.  The reference is unet_ref.augment_filter_sparse, shown equal to the dense product on the CPU for every case up to 300 nodes.

The trunk at depth 4, at ratio 1.0 and on a batch of graphs in different regimes, by the rule of tests/test_gpu_unet.py unchanged: kept
sets of every level exact, per tensor e <= max(4 x the float32 CPU restatement's e, 2e-5) against the float64 restatement (whose score
gaps are asserted first), two runs bit-equal, the one-segment form bit-equal.  FusedAdam at 24 and 17 tensors, GraphUNet at depth 4
through autograd."""
import ctypes as C

import pytest
import torch

import test_gpu_unet as TU
import unet_cases as UC
from test_gpu_unet import vp

pytestmark = pytest.mark.gpu

DRLGX_E_INVALID, DRLGX_E_CAPACITY = -1, -3
GUARD, FILL = 8, -5


# ---------------------------------------------------------------------------------------------------------------------
# augment and filter
# ---------------------------------------------------------------------------------------------------------------------
class AugmentCall(object):
    """One call of drlgx_unet_augment_filter with GUARD elements in front of and behind every output buffer, all prefilled with FILL."""

    def __init__(self, inp, dev, max_nodes=None):
        self.inp, self.cap, self.G = inp, int(inp["pooled_eoff"][-1]), len(inp["sizes"])
        self.max_nodes = inp["max_nodes"] if max_nodes is None else max_nodes
        self.d = [inp[k].to(dev) for k in ("edge_index", "edge_attr", "node_off", "edge_off", "pooled_off", "pooled_eoff")] + [inp["perm"].int().to(dev)]
        self.ei = torch.full((2 * self.cap + 2 * GUARD,), FILL, dtype=torch.int64, device=dev)
        self.ew = torch.full((self.cap + 2 * GUARD,), float(FILL), device=dev)
        self.counts = torch.full((self.G + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)

    def run(self):
        from drl_graph_exploration_amd import _lib
        ei, ew, node_off, edge_off, pooled_off, pooled_eoff, perm = self.d
        inside = lambda t: C.c_void_p(t.data_ptr() + GUARD * t.element_size())  # noqa: E731
        # n_edges = the columns of edge_index: row 1 begins there, whatever the graphs' slots cover
        rc = _lib.lib().drlgx_unet_augment_filter(None, sum(self.inp["sizes"]), ei.shape[1], vp(ei), vp(ew), self.G, vp(node_off), vp(edge_off),
                                                  self.max_nodes, vp(perm), vp(pooled_off), vp(pooled_eoff), self.cap, inside(self.ei),
                                                  inside(self.ew), inside(self.counts))
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        """(edge_index [2, cap], weights [cap], counts [G]) on the CPU, after checking that the guards are untouched."""
        ei, ew, counts = self.ei.cpu(), self.ew.cpu(), self.counts.cpu()
        for t in (ei, ew, counts):
            assert bool((t[:GUARD] == FILL).all()) and bool((t[-GUARD:] == FILL).all())  # nothing outside the buffers
        return ei[GUARD:-GUARD].view(2, self.cap), ew[GUARD:-GUARD], counts[GUARD:-GUARD]


def check_augment(inp, want, oe, ow, counts):
    """The assertions of test_augment_and_filter_is_exact, per graph.  Returns per graph its entries with the graph's offset taken off."""
    want_ei, want_ew, want_counts = want[:3]
    assert counts.tolist() == want_counts
    eoff, moff = inp["pooled_eoff"].tolist(), inp["pooled_off"].tolist()
    expect = sorted(zip(want_ei[0].tolist(), want_ei[1].tolist(), want_ew.tolist()))
    local, seen = [], 0
    for g in range(len(inp["sizes"])):
        a, n = eoff[g], want_counts[g]
        rows = list(zip(oe[0, a:a + n].tolist(), oe[1, a:a + n].tolist(), ow[a:a + n].tolist()))
        assert rows == sorted(rows) and len(set(r[:2] for r in rows)) == n, "graph %d" % g  # by (row, column), each once
        assert rows == expect[seen:seen + n], "graph %d" % g  # the reference's entries of this graph, exact weights
        assert bool((oe[:, a + n:eoff[g + 1]] == -1).all()), "graph %d" % g  # every slot from the count to the capacity is marked
        local.append([(r - moff[g], c - moff[g], w) for r, c, w in rows])
        seen += n
    assert seen == len(expect)
    return local


def run_augment_case(case, dev):
    inp = UC.augment_inputs(case)
    assert UC.regime(inp["sizes"], inp["ks"], inp["max_nodes"]) == [case["expect"][j] for j in inp["order"]]
    want = UC.augment_reference(inp)
    assert want[3] < UC.EXACT_LIMIT
    first, second = AugmentCall(inp, dev), AugmentCall(inp, dev)
    assert first.run() == 0 and second.run() == 0
    oe, ow, counts = first.outputs()
    local = check_augment(inp, want, oe, ow, counts)
    for a, b in zip(first.outputs(), second.outputs()):  # two calls are bit-equal
        assert torch.equal(a, b)
    return inp, oe, local


@pytest.mark.parametrize("case", UC.AUGMENT_CASES, ids=UC.AUGMENT_IDS)
def test_augment_and_filter_is_exact_where_passes_and_masks_wrap(case):
    inp, oe, _ = run_augment_case(case, torch.device("cuda", 0))
    if any(kind == "star" for kind, _, _ in case["graphs"]):
        assert not bool((oe == -1).any())  # the dense product fills the capacity


def test_a_graph_has_the_same_entries_wherever_it_stands_in_the_batch():
    """The mixed batch forwards and reversed: a graph's entries are the same apart from its offsets."""
    dev = torch.device("cuda", 0)
    entries = []
    for case in (c for c in UC.AUGMENT_CASES if c["id"] in ("mixed", "mixed-reversed")):
        inp, _, local = run_augment_case(case, dev)
        entries.append({j: local[g] for g, j in enumerate(inp["order"])})
    assert len(entries) == 2 and entries[0] == entries[1] and sum(len(v) for v in entries[0].values()) > 0


def test_augment_refuses_a_graph_beyond_the_cap_and_writes_nothing():
    dev = torch.device("cuda", 0)
    inp = UC.augment_inputs({"id": "beyond", "graphs": [("ring", UC.MAX_GRAPH_NODES + 1, 3)]})
    call = AugmentCall(inp, dev)
    assert call.run() == DRLGX_E_CAPACITY
    for t in (call.ei, call.ew, call.counts):
        assert bool((t == FILL).all())
    assert AugmentCall(inp, dev, max_nodes=0).run() == DRLGX_E_INVALID


# ---------------------------------------------------------------------------------------------------------------------
# the trunk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", UC.TRUNK_CASES, ids=UC.TRUNK_IDS)
def test_trunk_matches_the_float64_restatement_at_depth_4_and_ratio_1(case):
    from drl_graph_exploration_amd import _lib
    from drl_graph_exploration_amd.networks import unet_forward_raw
    dev = torch.device("cuda", 0)
    _, kind, hidden, depth, out_dim, with_mask, ratio, seed = case
    model, x, ei, ea, sizes, mask, d_out = UC.trunk_case(kind, hidden, depth, out_dim, with_mask, ratio, seed)
    N = x.shape[0]
    ref, levels = TU.reference(model, x, ei, ea, mask, d_out, sizes, torch.float64)
    TU.assert_gaps(levels)
    ref32, _ = TU.reference(model, x, ei, ea, mask, d_out, sizes, torch.float32)
    segs = None if sizes is None else TU.segments(sizes, ei, dev)
    got, kept = TU.hip_run(model, x, ei, ea, mask, d_out, dev, segs)
    again, _ = TU.hip_run(model, x, ei, ea, mask, d_out, dev, segs)
    assert len(kept) == depth == len(levels)
    for l, lv in enumerate(levels):  # the kept sets, exactly
        assert kept[l].tolist() == lv["perm"].tolist(), "level %d" % (l + 1)
        if ratio == 1.0:
            assert kept[l].tolist() == list(range(N))
    names, report = TU.names_of(model), []
    assert len(names) == 5 * depth + 5 == len(got) == len(ref)
    for name, g, r, r32 in zip(names, got, ref, ref32):
        assert g.shape == r.shape, name
        e, e32 = TU.rel(g, r), TU.rel(r32, r)
        report.append((name, e, e32, max(TU.FACTOR * e32, TU.FLOOR)))
    print("\n%s N=%d E=%d hidden=%d depth=%d out=%d mask=%s ratio=%g" % (kind, N, ei.shape[1], hidden, depth, out_dim, with_mask, ratio))
    for name, e, e32, bound in report:
        print("  %-22s hip %.3e  fp32 cpu %.3e  ratio %s  bound %.3e" % (name, e, e32, "%.2f" % (e / e32) if e32 > 0 else "-", bound))
    for name, e, e32, bound in report:
        assert e <= bound, (name, e, e32)
    for name, a, b in zip(names, got, again):  # deterministic reductions: two runs are bit-equal
        assert torch.equal(a, b), name
    if sizes is None and N > 1:  # one graph given as one segment: the same bits
        seg, _ = TU.hip_run(model, x, ei, ea, mask, d_out, dev, TU.segments([N], ei, dev))
        for name, a, b in zip(names, got, seg):
            assert torch.equal(a, b), name
    if depth == 4:  # the fourth kept set is level 4's; levels outside 1..depth are refused
        params = tuple(p.detach().to(dev) for p in model.trunk_parameters())
        _, saved = unet_forward_raw(x.to(dev), ei.to(dev), ea.to(dev), params, depth, ratio, None if mask is None else mask.to(dev), segs)
        ws, (n, E, _, hid, dep, rat, od, n_graphs, max_nodes) = saved[5], saved[6]
        out, count = torch.full((N,), -7, dtype=torch.int32, device=dev), C.c_int(-7)

        def kept_nodes(level):
            return _lib.lib().drlgx_unet_kept_nodes(C.c_void_p(_lib.stream_ptr(dev)), n, E, hid, dep, rat, od, vp(ws), ws.numel(), n_graphs, max_nodes,
                                                    level, vp(out), C.byref(count))

        assert kept_nodes(0) == DRLGX_E_INVALID and kept_nodes(5) == DRLGX_E_INVALID
        torch.cuda.synchronize()
        assert count.value == -7 and bool((out == -7).all())
        assert kept_nodes(4) == 0
        torch.cuda.synchronize()
        k4 = levels[3]["perm"].numel()
        assert count.value == k4 and out[:k4].cpu().tolist() == levels[3]["perm"].tolist() and bool((out[k4:] == -7).all())


def test_graph_unet_module_at_depth_4_matches_the_restatement_through_autograd():
    from drl_graph_exploration_amd.networks import GraphData, GraphUNet
    dev = torch.device("cuda", 0)
    x, ei, ea, sizes, batch = TU.module_batch()
    torch.manual_seed(UC.MODULE_SEED)
    model = GraphUNet(5, 1000, 1000, 4)
    assert len(list(model.parameters())) == 24
    d_out = torch.randn(x.shape[0], 1, generator=torch.Generator().manual_seed(8))
    m64, out64 = TU.module_reference(model, x, ei, ea, None, d_out, sizes, torch.float64)
    assert len(m64.levels) == 4
    TU.assert_gaps(m64.levels)
    m32, out32 = TU.module_reference(model, x, ei, ea, None, d_out, sizes, torch.float32)
    model.to(dev)
    q = model(GraphData(x.to(dev), ei.to(dev), ea.to(dev), batch.to(dev)), 0.0, batch=batch.to(dev))
    assert q.shape == (x.shape[0], 1)
    assert TU.rel(q.detach().cpu(), out64.double()) <= max(TU.FACTOR * TU.rel(out32.double(), out64.double()), TU.FLOOR)
    (q * d_out.to(dev)).sum().backward()
    for (name, p), r, r32 in zip(model.named_parameters(), m64.parameters(), m32.parameters()):
        assert p.grad is not None, name
        e, e32 = TU.rel(p.grad.cpu(), r.grad.double()), TU.rel(r32.grad.double(), r.grad.double())
        print("  %-22s hip %.3e  fp32 cpu %.3e" % (name, e, e32))
        assert e <= max(TU.FACTOR * e32, TU.FLOOR), name


# ---------------------------------------------------------------------------------------------------------------------
# optimiser
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tensors", [24, 17])
def test_fused_adam_steps_whole_groups_of_eight_and_two_groups_and_one(n_tensors):
    """A depth-4 GraphUNet has 24 parameters, three launches of eight; its first 17 are two launches of eight and one of one.  The bound
    of test_fused_adam_steps_nineteen_tensors_and_six_as_before against torch.optim.Adam."""
    from drl_graph_exploration_amd.networks import GraphUNet
    from drl_graph_exploration_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    torch.manual_seed(6)
    lr, clamp = 1e-3, 0.5
    model, twin = GraphUNet(5, 64, 64, 4).to(dev), GraphUNet(5, 64, 64, 4).to(dev)
    twin.load_state_dict(model.state_dict())
    ps, qs = list(model.parameters())[:n_tensors], list(twin.parameters())[:n_tensors]
    assert len(list(model.parameters())) == 24 and len(ps) == n_tensors
    opt, ref = FusedAdam(ps, lr=lr, grad_clamp=clamp), torch.optim.Adam(qs, lr=lr)
    gen = torch.Generator().manual_seed(9)
    start = [q.detach().clone() for q in qs]
    for step in range(3):
        opt.zero_grad()
        for p, q in zip(ps, qs):
            g = (torch.randn(p.shape, generator=gen) * 0.7).to(dev)  # some elements beyond the clamp
            p.grad.copy_(g)
            q.grad = g.clamp(-clamp, clamp)
        opt.step()
        ref.step()
        for i, (a, b) in enumerate(zip(ps, qs)):
            # one Adam step moves a parameter by at most ~lr: the two must agree to a small fraction of that
            assert float((a.detach() - b.detach()).abs().max()) < 2e-2 * lr * (step + 1), (step, i)
    assert opt.step_count == 3
    assert all(not torch.equal(a, b.detach()) for a, b in zip(start, ps))  # every tensor of every group was stepped
    for a, b in zip(list(model.parameters())[n_tensors:], list(twin.parameters())[n_tensors:]):
        assert torch.equal(a, b)  # and none behind them
