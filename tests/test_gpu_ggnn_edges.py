"""GPU tests of the HIP GG-NN trunk (csrc/k_ggnn.hip) where its CSR builds, thin products and tiles wrap: the cases of
tests/ggnn_cases.py through `ggnn_forward_raw` / `ggnn_backward_raw`, against tests/ggnn_ref.py in float64 on the CPU.

The rule of comparison is that of tests/test_gpu_ggnn.py: per tensor (the read-out and the seven gradients) e = max|delta| / max|ref|
is at most max(4 x the e of the same restatement in float32 on the CPU at that case, 2e-5); every case prints its ratios before it
asserts; two runs are bit-equal; rows in_dim.. of d_weight[0] are exactly zero.  The seven gradients are carved out of one NaN-filled
buffer with gaps of 64 floats: the gaps stay NaN and every gradient element is written.  Before any comparison the case's distance
from the ReLU's kink is asserted (ggnn_cases.gate_is_clear; the reasoning is in that module's docstring)."""
import ctypes as C
import math

import pytest
import torch

import ggnn_cases as GC

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 2e-5, 4.0
GAP = 64
PARAMS = ("weight", "w_ih", "w_hh", "b_ih", "b_hh", "Wf", "bf")


def rel(a, ref):
    d, m = float((a.double() - ref).abs().max()), float(ref.abs().max())
    return d / m if m > 0 else (0.0 if d == 0 else math.inf)


def one_float_in(t, dev):
    """A copy of t on the device that starts one float into a larger buffer: 4 bytes off every 16-byte boundary."""
    buf = torch.zeros(t.numel() + 8, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def hip_run(b, dev, ei, ea, segs=None, unaligned=()):
    """out and the seven gradients of one forward + backward call, on the CPU."""
    from drl_graph_exploration_amd.networks import ggnn_backward_raw, ggnn_forward_raw

    def put(name, t):
        return one_float_in(t.detach(), dev) if name in unaligned else t.detach().to(dev)

    params = tuple(put(name, p) for name, p in zip(PARAMS, b["model"].trunk_parameters()))
    x, d_out = put("x", b["x"]), put("d_out", b["d_out"])
    mask = None if b["mask"] is None else b["mask"].to(dev)
    out, saved = ggnn_forward_raw(x, ei.to(dev), ea.to(dev), params, mask, segs)
    sizes = [p.numel() for p in params]
    buf = torch.full((sum(sizes) + GAP * (len(sizes) + 1),), float("nan"), device=dev)
    grads, at = [], GAP
    for p, k in zip(params, sizes):
        grads.append(buf[at:at + k].view(p.shape))
        at += k + GAP
    ggnn_backward_raw(saved, d_out, tuple(grads))
    torch.cuda.synchronize()
    host, at = buf.cpu(), 0
    for name, k in zip(GC.NAMES[1:], sizes):  # the sentinels round every tensor are intact, every element of it is written
        assert bool(torch.isnan(host[at:at + GAP]).all()), "written in front of " + name
        assert not bool(torch.isnan(host[at + GAP:at + GAP + k]).any()), "unwritten elements of " + name
        at += GAP + k
    assert bool(torch.isnan(host[at:at + GAP]).all()), "written behind dbf"
    assert not bool(torch.isnan(out).any())
    return [out.cpu()] + [g.cpu().clone() for g in grads]


def compare(label, got, b):
    """Prints every tensor's figures, then asserts the bound; returns (largest e, largest HIP / float32 ratio)."""
    report = []
    for name, g, r, r32 in zip(GC.NAMES, got, b["ref"], b["ref32"]):
        assert g.shape == r.shape, name
        e, e32 = rel(g, r), rel(r32, r)
        report.append((name, e, e32, max(FACTOR * e32, FLOOR)))
    print("\n%s" % label)
    for name, e, e32, bound in report:
        print("  %-9s hip %.3e  fp32 cpu %.3e  ratio %s  bound %.3e" % (name, e, e32, "%.2f" % (e / e32) if e32 > 0 else "-", bound))
    worst = max(e for _, e, _, _ in report)
    ratio = max([e / e32 for _, e, e32, _ in report if e32 > 0] + [0.0])
    print("  FIGURES %s largest_e %.3e largest_ratio %.2f" % (label, worst, ratio))
    for name, e, e32, bound in report:
        assert e <= bound, (label, name, e, e32)
    in_dim = b["case"]["in_dim"]
    assert bool((got[1][0, in_dim:] == 0).all()), "rows in_dim.. of d_weight[0]"  # h_0's padding
    return worst, ratio


def bit_equal(what, a, b):
    for name, u, v in zip(GC.NAMES, a, b):
        assert torch.equal(u, v), (what, name)


@pytest.mark.parametrize("cid", GC.IDS)
def test_trunk_edge_case_matches_the_float64_restatement(cid):
    dev = torch.device("cuda", 0)
    case, b = GC.BY_ID[cid], GC.build(cid)
    assert GC.gate_is_clear(b), "an entry of h_L within tau of zero takes part in the comparison"
    sizes, counts = GC.graph_sizes(case)
    print("\n%s N=%d E=%d in=%d hidden=%d layers=%d out=%d mask=%s  tau %.3e, %d of %d entries within it (%.4f %%)  regime %r" % (
        cid, sum(sizes), sum(counts), case["in_dim"], case["hidden"], case["layers"], case["out_dim"], case["mask"], b["tau"], b["near"],
        b["h64"].numel(), 100.0 * b["near"] / b["h64"].numel(), GC.regime(case, case["ways"] == "both")))
    unaligned = case.get("unaligned", ())
    live = b["kind"] == 0
    generic = hip_run(b, dev, b["ref_ei"], b["ref_ea"], None, unaligned)  # (the generic build never sees a cross-graph edge: it would keep it)
    compare(cid + " generic", generic, b)
    if case["ways"] != "both":
        bit_equal("two runs", generic, hip_run(b, dev, b["ref_ei"], b["ref_ea"], None, unaligned))
        return
    seg = hip_run(b, dev, b["ei"], b["ea"], GC.segments(case, dev))  # the full slot list: dead slots and cross-graph edges are ignored
    compare(cid + " segments", seg, b)
    bit_equal("two runs", seg, hip_run(b, dev, b["ei"], b["ea"], GC.segments(case, dev)))
    bit_equal("one-launch against generic build", seg, generic)
    if not bool(live.all()):  # the generic build on the list with only the (-1, -1) slots left in
        keep = b["kind"] != 2
        bit_equal("dead slots in the generic build", hip_run(b, dev, b["ei"][:, keep], b["ea"][keep]), generic)


def test_wide_cases_sit_three_rows_past_the_tile_switches():
    """The two hidden 1000 cases of group C: asked of the library's own dispatch rule, not restated."""
    from drl_graph_exploration_amd import _lib
    tile = _lib.lib().drlgx_debug_gemm_tile_rows
    assert tile(GC.WIDE_GATE_ROWS, 3000, 1, 0) // 1000 == 128 and tile(GC.WIDE_GATE_ROWS - 1, 3000, 1, 0) // 1000 != 128
    assert all(tile(n, 3000, 1, 0) // 1000 != 128 for n in range(1, GC.WIDE_GATE_ROWS))
    assert tile(GC.WIDE_SQUARE_ROWS, 1000, 1, 0) != 64064 and all(tile(n, 1000, 1, 0) == 64064 for n in range(1, GC.WIDE_SQUARE_ROWS))
    rows = {sum(GC.graph_sizes(c)[0]) for c in GC.CASES if c["group"] == "C" and c["hidden"] == 1000}
    assert rows == {GC.WIDE_GATE_ROWS + 3, GC.WIDE_SQUARE_ROWS + 3}
    print("\ntiles: N x 3000 at %d rows %d, N x 1000 at %d rows %d" % (GC.WIDE_GATE_ROWS + 3, tile(GC.WIDE_GATE_ROWS + 3, 3000, 1, 0),
                                                                    GC.WIDE_SQUARE_ROWS + 3, tile(GC.WIDE_SQUARE_ROWS + 3, 1000, 1, 0)))


def test_unaligned_vector_operands_and_too_many_layers_are_refused():
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    buf = torch.zeros(1 << 10, device=dev)  # (zeros serve as x and as every parameter of the one valid call)
    ws = torch.empty(L.drlgx_ggnn_workspace_bytes(2, 0, 8, 2, 1), dtype=torch.uint8, device=dev)
    out = torch.full((2,), -7.0, device=dev)
    grads = torch.full((1 << 10,), -7.0, device=dev)
    p, off, pw, po, pg = (C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4), C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()),
                          C.c_void_p(grads.data_ptr()))
    assert buf.data_ptr() % 16 == 0

    def fwd(layers=2, weight=p, b_ih=p, b_hh=p, mask=None):
        return L.drlgx_ggnn_forward(None, 2, 0, 5, 8, layers, 1, p, None, None, weight, p, p, b_ih, b_hh, p, p, mask, po, pw, 0, None, None, 0)

    def bwd(layers=2):
        return L.drlgx_ggnn_backward(None, 2, 0, 5, 8, layers, 1, p, None, None, p, p, p, p, None, p, pg, pg, pg, pg, pg, pg, pg, pw)

    assert ws.numel() > 0
    assert fwd(mask=off) == -1 and fwd(weight=off) == -1 and fwd(b_ih=off) == -1 and fwd(b_hh=off) == -1  # DRLGX_E_INVALID
    assert fwd(layers=GC.MAX_LAYERS + 1) == -1 and bwd(layers=GC.MAX_LAYERS + 1) == -1
    assert L.drlgx_ggnn_workspace_bytes(2, 0, 8, GC.MAX_LAYERS + 1, 1) == 0 and L.drlgx_ggnn_workspace_bytes(2, 0, 8, GC.MAX_LAYERS, 1) > 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((grads == -7.0).all())  # nothing was launched
    assert fwd(mask=p) == 0  # the same call with the mask aligned is valid
    torch.cuda.synchronize()
    assert bool((out == 0).all())
