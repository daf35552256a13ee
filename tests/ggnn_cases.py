"""Cases of tests/test_gpu_ggnn_edges.py and their CPU checks in tests/test_ggnn_cpu.py: the GG-NN trunk (csrc/k_ggnn.hip) where the
one-launch CSR build's 256-strided loops take further passes, at its 2 048-edge dispatch limit, on repeated / self / ignored edges, at
every in_dim and at hidden sizes whose item rows cross waves and blocks, at node counts on both sides of the scan chunk, the thin
products' slice cap and the GEMM tile switches, at read-out widths round kThinOut, on unaligned operands and at 4 to 16 layers.

`regime` restates, in Python, which path a case reaches: the passes of k_csr_graphs_raw's three loops per graph, the build the dispatch
picks, k_scan2's chunk, thin_slices' slice count and rows per slice, gemm_tn_splitk's slice count.  It documents the table's `expect`
column (asserted on the CPU); it is not the reference of any result.  GEMM tile forms are asked of the library in the GPU test.

Every graph is drawn from a seed of its own (case family, position in the table's order), so that a batch given forwards and reversed
holds the same graphs; model, features, mask and d_out come from the case's `seed`.

The ReLU gate: the backward recovers it from Hm > 0, so an entry of h_L within float32 error of zero may legitimately flip, and one flip
moves a weight gradient far beyond the bound.  `build` therefore computes tau = TAU_FACTOR x the float32 restatement's largest absolute
error on h_L at that case (8 x the factor 4 that the comparison grants the HIP result) and
  * masked cases: zeroes the {0, 2} dropout mask wherever |h_L| < tau (at most MASKED_SHARE of the panel);
  * unmasked cases (small panels only): carry as `seed` the first seed of the searched range 1.. whose |h_L| >= tau everywhere."""
import functools
import zlib

import torch

import ggnn_ref

RAW_MAX_EDGES = 2048  # kRawMaxEdges
THIN_ROWS = 16  # kThinRows
THIN_OUT = 8  # kThinOut
MAX_LAYERS = 16  # kGgnnMaxLayers
DENSE_REF_NODES = 300  # the dense restatement runs up to here
TAU_FACTOR = 32.0
MASKED_SHARE = 1e-3
NAMES = ("out", "d_weight", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh", "dWf", "dbf")
# N x 3000 product: 128-column tiles from 641 rows on; N x 1000 product: off the 64 x 64 kernels from 1 025 rows on.  The GPU test asks
# the library's dispatch rule (drlgx_debug_gemm_tile_rows) that these are the smallest such counts; the cases take them + 3.
WIDE_GATE_ROWS, WIDE_SQUARE_ROWS = 641, 1025


# ---------------------------------------------------------------------------------------------------------------------
# the regime of a call
# ---------------------------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def part_floats(hidden):
    """carve: split-K partials of a hidden x hidden gradient (8 slices), or the thin products' (9 rows of 3 hidden, 128 slices)."""
    return max(8 * hidden * hidden, 128 * 9 * 3 * hidden)


def thin_slices(k, rows, n, part):
    """thin_slices of k_gcn_thin.hip: (slice count, rows per slice)."""
    nb = min(128, _ceil(k, 8))
    nb = max(1, min(nb, part // (rows * n)))
    rpb = _ceil(k, nb)
    return _ceil(k, rpb), rpb


def splitk_slices(m, n, k, part, max_splits=8):
    """gemm_tn_splitk: the K-slices of an m x n weight gradient over k nodes."""
    tiles = _ceil(m, 64) * _ceil(n, 64)
    splits = min(max_splits, part // (m * n))
    splits = max(1, min(splits, _ceil(1024, tiles), _ceil(k, 256)))
    kps = _ceil(_ceil(k, splits), 16) * 16
    return _ceil(k, kps)


def regime(case, with_segments):
    """What one forward + backward call of the case reaches:
      build   "one-launch" (k_csr_graphs_raw) or "generic" (count / scan / fill / sort / k_csr_raw)
      csr     one-launch only: per graph the passes of (the node loops, the edge loop, the rank loop)
      scan    generic only: k_scan2's elements per thread
      thin    (slices, rows per slice) of layer 0's thin_tn over d(gh): in_dim + 1 rows of 3 hidden
      splitk  K-slices of a hidden x hidden weight gradient"""
    sizes, counts = graph_sizes(case)
    n, hidden = sum(sizes), case["hidden"]
    part = part_floats(hidden)
    one_launch = with_segments and max(counts) <= RAW_MAX_EDGES
    out = {"build": "one-launch" if one_launch else "generic",
           "thin": thin_slices(n, case["in_dim"] + 1, 3 * hidden, part),
           "splitk": splitk_slices(hidden, hidden, n, part)}
    if one_launch:
        out["csr"] = [(_ceil(ng, 256), _ceil(eg, 256), _ceil(eg, 256)) for ng, eg in zip(sizes, counts)]
    else:
        out["scan"] = _ceil(n, 1024)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# graphs (local node ids)
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


def _weights(m, n, gen):
    """0.1 .. 3.0 as tests/test_gpu_ggnn.py draws them, scaled down where a node has more than four edges on average (the gates
    would saturate and every gradient vanish)."""
    return (torch.rand(m, generator=gen) * 2.9 + 0.1) * min(1.0, 4.0 * max(n, 1) / max(m, 1))


def random_graph(n, m, gen):
    """m directed edges without self loops, asymmetric."""
    if m == 0:
        return torch.zeros(2, 0, dtype=torch.long), torch.zeros(0)
    src = torch.randint(0, n, (m,), generator=gen)
    dst = (src + 1 + torch.randint(0, n - 1, (m,), generator=gen)) % n
    return torch.stack([src, dst]), _weights(m, n, gen)


def repeats_graph(n, m, gen):
    """3 n random edges (m is what comes out: see A5); every fifth given three more times, each time with a weight of its own; one
    explicit self loop on every third node; a tenth of the weights 0, a tenth negative; shuffled, so that the copies of an edge sit
    among the other edges of their row."""
    ei, _ = random_graph(n, 3 * n, gen)
    again = ei[:, ::5]
    loops = torch.arange(0, n, 3)
    ei = torch.cat([ei, again, again, again, torch.stack([loops, loops])], 1)
    assert ei.shape[1] == m
    ei = ei[:, torch.randperm(m, generator=gen)]
    ew = _weights(m, n, gen)
    kind = torch.randperm(m, generator=gen)
    ew[kind[:m // 10]] = 0.0
    ew[kind[m // 10:2 * (m // 10)]] *= -1.0
    return ei, ew


def _repeats_edges(n):
    return 3 * n + 3 * _ceil(3 * n, 5) + _ceil(n, 3)


GRAPHS = {"rand": random_graph, "repeats": repeats_graph}


def _foreign(ei, ew, n_own, off_other, n_other, gen):
    """The graph's slots with a tenth overwritten by (-1, -1) and a weight that would show, and six edges with one endpoint in the
    other graph (ids relative to this graph's first node), three in either direction.  Returns (edge_index, weights, kind per slot:
    0 an edge of the graph, 1 a dead slot, 2 a cross-graph edge)."""
    ei, ew = ei.clone(), ew.clone()
    kind = torch.zeros(ei.shape[1], dtype=torch.long)
    dead = torch.randperm(ei.shape[1], generator=gen)[:ei.shape[1] // 10]
    ei[:, dead], ew[dead], kind[dead] = -1, 7.0, 1
    inside = torch.randint(0, n_own, (6,), generator=gen)
    outside = off_other + torch.randint(0, n_other, (6,), generator=gen)
    cross = torch.cat([torch.stack([inside[:3], outside[:3]]), torch.stack([outside[3:], inside[3:]])], 1)
    ei, ew, kind = torch.cat([ei, cross], 1), torch.cat([ew, torch.full((6,), 5.0)]), torch.cat([kind, torch.full((6,), 2)])
    order = torch.randperm(ei.shape[1], generator=gen)
    return ei[:, order], ew[order], kind[order]


def graph_sizes(case):
    """(node counts, edge slots) per graph, in the order of the call."""
    spec = case["graphs"][::-1] if case.get("reversed") else case["graphs"]
    extra = 6 if case.get("foreign") else 0
    return [n for _, n, _ in spec], [m + extra for _, _, m in spec]


def edges(case):
    """(edge_index [2, E] grouped by graph, edge_attr [E], kind per slot) of the whole call, global node ids; -1 stays -1."""
    spec = list(enumerate(case["graphs"]))
    if case.get("reversed"):
        spec.reverse()
    sizes = [n for _, (_, n, _) in spec]
    eis, ews, kinds, off = [torch.zeros(2, 0, dtype=torch.long)], [torch.zeros(0)], [torch.zeros(0, dtype=torch.long)], 0
    for pos, (j, (kind, n, m)) in enumerate(spec):
        gen = _gen(case["family"], kind, n, m, j)
        ei, ew = GRAPHS[kind](n, m, gen)
        k = torch.zeros(m, dtype=torch.long)
        if case.get("foreign"):  # two graphs
            other = 1 - pos
            ei, ew, k = _foreign(ei, ew, n, (sizes[0] if other else -sizes[0]), sizes[other], gen)
        eis.append(torch.where(k == 1, ei, ei + off))
        ews.append(ew)
        kinds.append(k)
        off += n
    return torch.cat(eis, 1), torch.cat(ews), torch.cat(kinds)


def segments(case, dev=None):
    """(n_graphs, node_off, edge_off, max edges of a graph) as drlgx_ggnn_forward takes them."""
    sizes, counts = graph_sizes(case)
    node_off = torch.tensor([0] + sizes).cumsum(0).int()
    edge_off = torch.tensor([0] + counts).cumsum(0).int()
    if dev is not None:
        node_off, edge_off = node_off.to(dev), edge_off.to(dev)
    return len(sizes), node_off, edge_off, max(counts)


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def _case(cid, group, graphs, expect, *, in_dim=5, hidden=8, layers=2, out_dim=1, mask=True, seed=1, ways="generic", **more):
    """graphs: [(kind, nodes, edge slots)].  ways: "both" - with segments, without, and the two bit-equal - or "generic".
    expect: what `regime` gives, as (build with segments, csr passes per graph, scan chunk, thin, splitk); see _expect."""
    c = {"id": cid, "group": group, "family": more.pop("family", cid), "graphs": graphs, "expect": expect, "in_dim": in_dim, "hidden": hidden,
         "layers": layers, "out_dim": out_dim, "mask": mask, "seed": seed, "ways": ways}
    c.update(more)
    return c


def expected(case):
    """The `expect` column spelt out as the two `regime` dicts (with segments: None for a generic-only case; without)."""
    build, csr, scan, thin, splitk = case["expect"]
    seg = None
    if case["ways"] == "both":
        seg = {"build": build, "thin": thin, "splitk": splitk}
        seg.update({"csr": csr} if build == "one-launch" else {"scan": scan})
    return seg, {"build": "generic", "scan": scan, "thin": thin, "splitk": splitk}


def _rand(n, per_node=4):
    return [("rand", n, per_node * n)]


ONE, GEN = "one-launch", "generic"
A4 = [("rand", 1, 0), ("rand", 0, 0), ("rand", 300, 900), ("rand", 2, 1), ("rand", 40, 513), ("rand", 257, 771)]
A4_CSR = [(1, 0, 0), (0, 0, 0), (2, 4, 4), (1, 1, 1), (1, 3, 3), (2, 4, 4)]

CASES = (
    # ---- A: the one-launch CSR build -------------------------------------------------------------------------------
    # A1 edge and rank loops: 1, 1, 2, 3 passes
    [_case("A1-e%d" % m, "A", [("rand", 40, m)], (ONE, [(1, p, p)], 1, (5, 8), 1), ways="both") for m, p in ((255, 1), (256, 1), (257, 2), (513, 3))]
    # A2 node loops: 1, 1, 2, 3 passes (three edges per node: 3 to 8 passes of the edge loops)
    + [_case("A2-n%d" % n, "A", _rand(n, 3), (ONE, [(p, q, q)], 1, t, s), ways="both")
       for n, p, q, t, s in ((255, 1, 3, (32, 8), 1), (256, 1, 3, (32, 8), 1), (257, 2, 4, (33, 8), 2), (600, 3, 8, (75, 8), 3))]
    # A3 the cap: 2 047 and 2 048 edges in one launch, 2 049 generic by dispatch; a batch with one such graph goes generic as a whole
    + [_case("A3-e%d" % m, "A", [("rand", 700, m)], (b, [(3, 8, 8)], 1, (88, 8), 3), ways="both") for m, b in ((2047, ONE), (2048, ONE), (2049, GEN))]
    + [_case("A3-5+11+e2049", "A", [("rand", 5, 15), ("rand", 11, 33), ("rand", 700, 2049)], (GEN, None, 1, (90, 8), 3), ways="both")]
    # A4 graphs in different regimes in one call, and in reversed order (each order against the reference only)
    + [_case("A4-mixed", "A", A4, (ONE, A4_CSR, 1, (75, 8), 3), ways="both"),
       _case("A4-mixed-reversed", "A", A4, (ONE, A4_CSR[::-1], 1, (75, 8), 3), ways="both", family="A4-mixed", reversed=True)]
    # A5 rank tie-break and self weight: repeated edges, explicit self loops, zero and negative weights
    + [_case("A5-n64", "A", [("repeats", 64, _repeats_edges(64))], (ONE, [(1, 2, 2)], 1, (8, 8), 1), ways="both"),
       _case("A5-n257", "A", [("repeats", 257, _repeats_edges(257))], (ONE, [(2, 6, 6)], 1, (33, 8), 2), ways="both")]
    # A6 ignored edges: dead slots and edges into the other graph (see the GPU test for the three lists)
    + [_case("A6-foreign-200+33", "A", [("rand", 200, 600), ("rand", 33, 99)], (ONE, [(1, 3, 3), (1, 1, 1)], 1, (30, 8), 1), ways="both", foreign=True)]
    # A7 no edge at all
    + [_case("A7-3+2-e0", "A", [("rand", 3, 0), ("rand", 2, 0)], (ONE, [(1, 0, 0), (1, 0, 0)], 1, (1, 5), 1), ways="both")]
    # ---- B: in_dim and hidden; N = 19 (one full block of kThinRows and three rows), 3 layers -------------------------
    + [_case("B-in%d-h%d" % (i, h), "B", _rand(19), (GEN, None, 1, (3, 7), 1), in_dim=i, hidden=h, layers=3, mask=m, seed=s, searched=r)
       for i, h, m, s, r in ((1, 8, True, 1, None), (3, 8, True, 1, None), (4, 8, True, 1, None), (8, 8, False, 1, (1, 1)), (1, 4, True, 1, None),
                             (4, 4, False, 1, (1, 1)))]
    + [_case("B-in5-h%d-o%d" % (h, o), "B", _rand(19), (GEN, None, 1, (3, 7), 1), hidden=h, layers=3, out_dim=o, mask=m, seed=s, searched=r)
       for h, o, m, s, r in ((12, 1, False, 1, (1, 1)), (12, 100, True, 1, None), (20, 1, True, 1, None), (68, 1, True, 1, None),
                             (260, 1, True, 1, None), (260, 100, True, 1, None), (1028, 1, True, 1, None))]
    # ---- C: node counts; four edges per node -----------------------------------------------------------------------
    + [_case("C-n%d" % n, "C", _rand(n), (GEN, None, c, t, s))
       for n, c, t, s in ((15, 1, (2, 8), 1), (16, 1, (2, 8), 1), (17, 1, (3, 6), 1), (255, 1, (32, 8), 1), (256, 1, (32, 8), 1),
                          (257, 1, (33, 8), 2), (1023, 1, (128, 8), 4), (1024, 1, (128, 8), 4), (1025, 2, (114, 9), 5), (2049, 3, (121, 17), 8))]
    + [_case("C-h1000-n%d-o%d" % (n, o), "C", _rand(n), (GEN, None, c, t, s), hidden=1000, layers=3, out_dim=o)
       for n, o, c, t, s in ((WIDE_GATE_ROWS + 3, 1, 1, (81, 8), 3), (WIDE_SQUARE_ROWS + 3, 100, 2, (115, 9), 4))]
    # ---- D: read-out widths round kThinOut, and unaligned operands; N = 70, hidden 68, 3 layers ---------------------
    + [_case("D-o%d" % o, "D", _rand(70), (GEN, None, 1, (9, 8), 1), hidden=68, layers=3, out_dim=o) for o in (2, 7, 8, 9, 12, 16, 17)]
    + [_case("D-h1000-o%d" % o, "D", _rand(71), (GEN, None, 1, (9, 8), 1), hidden=1000, layers=3, out_dim=o) for o in (8, 9)]
    + [_case("D-unaligned-%s-o%d" % ("+".join(u), o), "D", _rand(70), (GEN, None, 1, (9, 8), 1), hidden=68, layers=3, out_dim=o, unaligned=u,
             family="D-unaligned")
       for u, o in ((("Wf",), 1), (("Wf",), 8), (("Wf",), 9), (("Wf",), 100), (("bf",), 100), (("w_ih", "w_hh"), 1), (("x",), 1), (("d_out",), 100))]
    # ---- E: layers; N = 33 -------------------------------------------------------------------------------------------
    + [_case("E-L%d" % l, "E", _rand(33), (GEN, None, 1, (5, 7), 1), layers=l) for l in (4, 5, 16)]
)
IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references of a case
# ---------------------------------------------------------------------------------------------------------------------
def _features(case, seed):
    """(model, x, raw {0, 2} mask or None, d_out) from the seed."""
    sizes, _ = graph_sizes(case)
    n, hidden, in_dim, out_dim = sum(sizes), case["hidden"], case["in_dim"], case["out_dim"]
    gen = _gen("features", case["family"], hidden, case["layers"], in_dim, out_dim, seed)
    torch.manual_seed(100 * seed + hidden + case["layers"] + out_dim)
    model = ggnn_ref.RefGGNN(hidden, case["layers"], out_dim)  # random weights: the modules' own init
    x = torch.randn(n, in_dim, generator=gen)
    if in_dim == 5:
        x[:, 4] = torch.randint(-1, 2, (n,), generator=gen).float()
    mask = (torch.rand(n, hidden, generator=gen) >= 0.5).float() * 2.0 if case["mask"] else None
    return model, x, mask, torch.randn(n, out_dim, generator=gen)


def _at(model, dtype, dense=False):
    g = model.gconv1
    m = ggnn_ref.RefGGNN(g.out_channels, g.num_layers, model.fully_con1.out_features, dense=dense).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in model.state_dict().items()})
    return m


def last_states(model, x, ei, ea):
    """(h_L of the float64 restatement, of the float32 one as float64, tau)."""
    with torch.no_grad():
        h64 = _at(model, torch.float64).gconv1(x.double(), ei, ea.double())
        h32 = _at(model, torch.float32).gconv1(x, ei, ea).double()
    return h64, h32, TAU_FACTOR * float((h32 - h64).abs().max())


def reference(model, x, ei, ea, mask, d_out, dtype, dense=False):
    """out and the seven gradients of sum(out * d_out) from the restatement at `dtype`, as float64 tensors."""
    m = _at(model, dtype, dense)
    out = m(x.to(dtype), ei, ea.to(dtype), None if mask is None else mask.to(dtype))
    (out * d_out.to(dtype)).sum().backward()
    return [out.detach().double()] + [p.grad.double() for p in m.trunk_parameters()]


def seed_is_clear(case, seed):
    """Unmasked cases: every |h_L| >= tau at this seed."""
    ei, ea, kind = edges(case)
    model, x, _, _ = _features(case, seed)
    h64, _, tau = last_states(model, x, ei[:, kind == 0], ea[kind == 0])
    return float(h64.abs().min()) >= tau


@functools.lru_cache(maxsize=2)
def build(cid):
    """Everything the tests need of a case, computed once: the full slot list (`ei`, `ea`, `kind`), the filtered list the reference gets
    (`ref_ei`, `ref_ea`), model, x, mask (after the tau rule), d_out, tau, h64, `masked` (entries the rule zeroed) and the references
    `ref` (float64) and `ref32` (float32) on the filtered list.  Treat it as read-only."""
    case = BY_ID[cid]
    ei, ea, kind = edges(case)
    ref_ei, ref_ea = ei[:, kind == 0], ea[kind == 0]
    model, x, mask, d_out = _features(case, case["seed"])
    h64, _, tau = last_states(model, x, ref_ei, ref_ea)
    near = h64.abs() < tau
    masked = 0
    if mask is not None:
        masked = int((near & (mask != 0)).sum())
        mask = torch.where(near, torch.zeros_like(mask), mask)
    return {"case": case, "ei": ei, "ea": ea, "kind": kind, "ref_ei": ref_ei, "ref_ea": ref_ea, "model": model, "x": x, "mask": mask,
            "d_out": d_out, "tau": tau, "h64": h64, "near": int(near.sum()), "masked": masked,
            "ref": reference(model, x, ref_ei, ref_ea, mask, d_out, torch.float64),
            "ref32": reference(model, x, ref_ei, ref_ea, mask, d_out, torch.float32)}


def gate_is_clear(b):
    """The condition both test files assert before any comparison: no live entry of the panel sits within tau of the ReLU's kink -
    unmasked: none at all; masked: those there are have been masked, and they are at most MASKED_SHARE of the panel."""
    if b["mask"] is None:
        return b["near"] == 0
    live = (b["h64"].abs() < b["tau"]) & (b["mask"] != 0)
    return not bool(live.any()) and b["near"] <= MASKED_SHARE * b["h64"].numel()
