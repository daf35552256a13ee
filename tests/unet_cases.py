"""Cases of tests/test_gpu_unet_edges.py and their CPU checks in tests/test_unet_cpu.py: the g-U-Net pooling kernels (csrc/k_unet.hip)
where the augment-and-filter kernel's row passes and bit masks wrap, and the trunk at depth 4, at ratio 1.0 and on a batch whose graphs
sit in different regimes at once.

`regime` restates, in Python, how many kept rows k_unet_augment has in flight (T) and how many passes it makes over a graph's kept rows:
`launch_lds_words` is launch_augment's sizing of the dynamic LDS, `rows_in_flight` the kernel's own T.  It documents which regime a case
reaches (the table's `expect` column, asserted on the CPU); it is not the reference of any result.

Every graph of an augment case has small-integer weights (float32 is exact) and is drawn from a seed of its own, so that a batch given
forwards and reversed holds the same graphs."""
import zlib

import torch

import unet_ref

LDS_WORDS = 32 * 1024  # kUnetLdsWords
MAX_GRAPH_NODES = 4096  # kUnetMaxGraphNodes
DENSE_REF_NODES = 300  # the dense reference runs up to here; beyond it the sparse restatement alone
EXACT_LIMIT = float(1 << 24)  # float32 holds every integer below
BOUNDARY_COLUMNS = (31, 32, 63, 64)  # both sides of the first two mask-word boundaries


# ---------------------------------------------------------------------------------------------------------------------
# the regime of a launch: rows in flight and passes
# ---------------------------------------------------------------------------------------------------------------------
def launch_lds_words(max_nodes, max_kept):
    """launch_augment: as many rows in flight as the largest graph keeps (256 at most), while they fit the budget."""
    nw = (max_nodes + 31) >> 5
    want = max_nodes + min(256, max(max_kept, 1)) * (2 * max_nodes + 2 * nw)
    return min(LDS_WORDS, max(want, 64))


def rows_in_flight(ng, lds_words):
    """k_unet_augment: T of a graph of ng nodes (two dense rows and two bit masks per thread behind the ng words of s_new)."""
    per_row = 2 * ng + 2 * ((ng + 31) >> 5)
    return min(256, (lds_words - ng) // per_row) if per_row > 0 else 0


def regime(sizes, ks, max_nodes):
    """[(T, passes)] of the graphs of one drlgx_unet_augment_filter call (the entry passes max_graph_nodes as the kept bound too)."""
    lds = launch_lds_words(max_nodes, max_nodes)
    out = []
    for n, k in zip(sizes, ks):
        t = rows_in_flight(n, lds)
        assert t >= 1 and n + t * (2 * n + 2 * ((n + 31) >> 5)) <= lds  # the kernel's rows stay inside its LDS
        out.append((t, -(-k // t)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# graphs (local node ids) and kept rows
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


def _weights(m, gen):
    return torch.randint(1, 4, (m,), generator=gen).float()


def ring_chords(n, gen):
    """A directed ring and one to three chords per node: 2 to 4 edges per node, in a shuffled order."""
    if n < 2:
        return torch.zeros(2, 0, dtype=torch.long), torch.zeros(0)
    nodes = torch.arange(n)
    extra = torch.repeat_interleave(nodes, torch.randint(1, 4, (n,), generator=gen))
    src = torch.cat([nodes, extra])
    dst = torch.cat([(nodes + 1) % n, (extra + 1 + torch.randint(0, n - 1, (extra.numel(),), generator=gen)) % n])
    order = torch.randperm(src.numel(), generator=gen)
    return torch.stack([src, dst])[:, order], _weights(src.numel(), gen)


def star_both(n, gen):
    """Hub 0 to every leaf and back: (A + I)^2 is dense."""
    leaves, hub = torch.arange(1, n), torch.zeros(n - 1, dtype=torch.long)
    ei = torch.cat([torch.stack([leaves, hub]), torch.stack([hub, leaves])], 1)
    return ei[:, torch.randperm(ei.shape[1], generator=gen)], _weights(ei.shape[1], gen)


def with_repeats(n, gen):
    """ring_chords with a quarter of its edges given a second and a third time, and explicit self loops on every fifth node."""
    ei, ew = ring_chords(n, gen)
    again = ei[:, torch.randperm(ei.shape[1], generator=gen)[:ei.shape[1] // 4]]
    loops = torch.arange(0, n, 5)
    ei = torch.cat([ei, again, again, torch.stack([loops, loops])], 1)
    return ei[:, torch.randperm(ei.shape[1], generator=gen)], _weights(ei.shape[1], gen)


GRAPHS = {"ring": ring_chords, "star": star_both, "repeats": with_repeats}


def kept_rows(n, keep, gen):
    """Ascending local ids of the kept nodes.  "all"; an int: that many, at random; "with" / "without": a random half (ceil) that
    contains / lacks every column of BOUNDARY_COLUMNS the graph has."""
    if keep == "all":
        return torch.arange(n)
    edge = [c for c in BOUNDARY_COLUMNS if c < n]
    if isinstance(keep, int):
        must, pool, k = [], list(range(n)), keep
    elif keep == "with":
        must, pool, k = edge, [i for i in range(n) if i not in edge], (n + 1) // 2
    else:
        must, pool, k = [], [i for i in range(n) if i not in edge], (n + 1) // 2
    pick = torch.randperm(len(pool), generator=gen)[:k - len(must)].tolist()
    return torch.tensor(sorted(must + [pool[i] for i in pick]), dtype=torch.long)


# ---------------------------------------------------------------------------------------------------------------------
# the augment-and-filter cases
# ---------------------------------------------------------------------------------------------------------------------
def _one(n, keep, t, passes, kind="ring"):
    name = "%s%d-keep_%s" % ("" if kind == "ring" else kind + "-", n, keep)
    return {"id": name, "graphs": [(kind, n, keep)], "expect": [(t, passes)]}


MIXED = [("ring", 1, "all"), ("ring", 2, "all"), ("ring", 61, "all"), ("ring", 62, "all"), ("ring", 33, "with"), ("ring", 200, "all"),
         ("ring", 130, "all")]
MIXED_EXPECT = [(256, 1), (256, 1), (256, 1), (255, 1), (256, 1), (78, 3), (120, 2)]

AUGMENT_CASES = (
    # mask words of 1, 2, 3 and 4 words; the LDS holds every row (T = n, one pass)
    [_one(n, keep, n, 1) for n in (31, 32, 33, 63, 64, 65, 96, 97) for keep in ("all", "with", "without")]
    # the first sizes whose rows no longer fit at once (125 is the last that does)
    + [_one(125, "all", 125, 1), _one(126, "all", 125, 2), _one(128, "all", 123, 2), _one(129, "all", 121, 2)]
    # T around a wave
    + [_one(246, "all", 64, 4), _one(247, "all", 63, 4)]
    # T far from a multiple of 64: whole passes, one row more, every row
    + [_one(200, 78, 78, 1), _one(200, 79, 78, 2), _one(200, 156, 78, 2), _one(200, 157, 78, 3), _one(200, "all", 78, 3)]
    + [_one(257, "all", 61, 5), _one(1025, 15, 15, 1), _one(1025, 16, 15, 2), _one(1025, 31, 15, 3)]
    # the cap: three rows in flight
    + [_one(n, k, 3, p) for n in (4095, 4096) for k, p in ((3, 1), (4, 2), (7, 3))]
    # the LDS sized by another graph of the call
    + [{"id": "mixed", "graphs": MIXED, "expect": MIXED_EXPECT},
       {"id": "mixed-reversed", "graphs": MIXED, "expect": MIXED_EXPECT, "reversed": True},
       {"id": "ring61-lds_of_200", "graphs": [("ring", 61, "all")], "max_nodes": 200, "expect": [(256, 1)]},
       {"id": "ring62-lds_of_200", "graphs": [("ring", 62, "all")], "max_nodes": 200, "expect": [(255, 1)]}]
    # input slots that hold no edge of the graph, and a row stride beyond the slots in use (what levels >= 2 of the trunk read)
    + [{"id": "foreign-200+33", "graphs": [("ring", 200, 157), ("ring", 33, "all")], "expect": [(78, 3), (256, 1)], "foreign": True}]
    # the dense product: the output fills its capacity k (k - 1)
    + [_one(130, "all", 120, 2, "star"), _one(200, "all", 78, 3, "star")]
    # repeated edges and explicit self loops
    + [_one(64, "all", 64, 1, "repeats"), _one(200, 157, 78, 3, "repeats")]
)
AUGMENT_IDS = [c["id"] for c in AUGMENT_CASES]


def _foreign_slots(ei, ew, n0, n1, gen):
    """Graph 0's slots (local ids; graph 1's nodes follow at n0 ..) as a deeper level hands them on: a tenth overwritten by (-1, -1) with
    a weight that would show, and edges with one endpoint in graph 1, in either direction."""
    ei, ew = ei.clone(), ew.clone()
    dead = torch.randperm(ei.shape[1], generator=gen)[:ei.shape[1] // 10]
    ei[:, dead] = -1
    ew[dead] = 7.0
    inside, outside = torch.randint(0, n0, (12,), generator=gen), n0 + torch.randint(0, n1, (12,), generator=gen)
    cross = torch.cat([torch.stack([inside[:6], outside[:6]]), torch.stack([outside[6:], inside[6:]])], 1)
    ei, ew = torch.cat([ei, cross], 1), torch.cat([ew, torch.full((12,), 5.0)])
    order = torch.randperm(ei.shape[1], generator=gen)
    return ei[:, order], ew[order]


def augment_inputs(case):
    """What one call of drlgx_unet_augment_filter takes, on the CPU: sizes, ks, max_nodes, node_off / edge_off / pooled_off / pooled_eoff
    (int32), perm (int64, global ids), edge_index [2, E] with its first `used` slots in use and edge_attr [E]; `order`: the position
    of every graph in the table's own order."""
    spec = list(enumerate(case["graphs"]))
    if case.get("reversed"):
        spec.reverse()
    sizes = [n for _, (_, n, _) in spec]
    eis, ews, perms, ks, off = [], [], [], [], 0
    for j, (kind, n, keep) in spec:
        gen = _gen(kind, n, keep, j)
        ei, ew = GRAPHS[kind](n, gen)
        kept = kept_rows(n, keep, gen)
        if case.get("foreign") and j == 0:
            ei, ew = _foreign_slots(ei, ew, n, sizes[1], gen)
        eis.append(torch.where(ei >= 0, ei + off, ei))
        ews.append(ew)
        perms.append(kept + off)
        ks.append(int(kept.numel()))
        off += n
    ei, ew = torch.cat(eis, 1), torch.cat(ews)
    used = ei.shape[1]
    if case.get("foreign"):  # slots behind the last graph's: edges of graph 0 by their ids, but no graph's slots
        tail = torch.stack([torch.arange(37), (torch.arange(37) + 2) % sizes[0]])
        ei, ew = torch.cat([ei, tail], 1), torch.cat([ew, torch.full((37,), 5.0)])

    def prefix(v):
        return torch.tensor([0] + list(v)).cumsum(0).int()

    return {"sizes": sizes, "ks": ks, "max_nodes": case.get("max_nodes", max(sizes)), "order": [j for j, _ in spec],
            "node_off": prefix(sizes), "edge_off": prefix(e.shape[1] for e in eis), "pooled_off": prefix(ks),
            "pooled_eoff": prefix(k * (k - 1) for k in ks), "perm": torch.cat(perms), "edge_index": ei, "edge_attr": ew, "used": used}


def augment_reference(inp, dense=False):
    """(edge_index, weights (float64), counts per graph, largest entry of (A + I)^2 over the kept rows) of the slots in use."""
    ei, ew = inp["edge_index"][:, :inp["used"]], inp["edge_attr"][:inp["used"]].double()
    if dense:
        return unet_ref.augment_filter(ei, ew, inp["sizes"], inp["perm"], inp["ks"])
    rows = unet_ref.augment_rows_sparse(ei, ew, inp["sizes"], inp["perm"], inp["ks"])
    largest = max([max(acc.values()) for g in rows for _, acc in g] + [0.0])
    return unet_ref.augment_filter_sparse(ei, ew, inp["sizes"], inp["perm"], inp["ks"]) + (largest,)


# ---------------------------------------------------------------------------------------------------------------------
# the trunk cases
# ---------------------------------------------------------------------------------------------------------------------
def _random_edges(n, m, gen):
    src = torch.randint(0, n, (m,), generator=gen)
    dst = (src + 1 + torch.randint(0, n - 1, (m,), generator=gen)) % n
    return torch.stack([src, dst]), torch.rand(m, generator=gen) * 2.9 + 0.1


def _batch_of(sizes, gen, per_node=3):
    parts, ws, off = [torch.zeros(2, 0, dtype=torch.long)], [torch.zeros(0)], 0
    for k in sizes:
        if k > 1:
            e, w = _random_edges(k, per_node * k, gen)
            parts.append(e + off)
            ws.append(w)
        off += k
    return torch.cat(parts, 1), torch.cat(ws)


TRUNK_GRAPHS = {  # node counts per graph; None: one graph given without boundaries
    "single": None, "two": None, "fan": None, "n130": None, "n200": None,
    "batch": [5, 1, 11, 2],
    "mixed": [200, 3, 64, 65, 1, 130],
}


def trunk_graph(kind, gen):
    """(n, edge_index, edge_attr, node counts per graph or None)"""
    sizes = TRUNK_GRAPHS[kind]
    if kind == "single":
        return 1, torch.zeros(2, 0, dtype=torch.long), torch.zeros(0), None
    if kind == "two":
        return 2, torch.tensor([[0], [1]]), torch.tensor([1.3]), None
    if kind == "fan":
        return 3, torch.tensor([[0, 0], [1, 2]]), torch.tensor([0.7, 2.3]), None
    if kind == "n200":
        # a ring with one short chord per node: its square stays banded, so the pooled graphs of four levels keep nodes that differ (on
        # random edges the fourth power is nearly complete, every deep score is the same number and no seed clears the gap)
        nodes = torch.arange(200)
        src, dst = torch.cat([nodes, nodes]), torch.cat([nodes + 1, nodes + torch.randint(2, 4, (200,), generator=gen)]) % 200
        return 200, torch.stack([src, dst]), torch.rand(400, generator=gen) * 2.9 + 0.1, None
    if sizes is None:
        n = int(kind[1:])
        return (n,) + _random_edges(n, 4 * n, gen) + (None,)
    return (sum(sizes),) + _batch_of(sizes, gen) + (sizes,)


# id, kind, hidden, depth, out_dim, mask, ratio, seed.  The seed is the first of the searched range whose float64 reference keeps every
# k-th place of every level and graph clear by GAP x the level's largest |score| (tests/test_gpu_unet.py: assert_gaps); where every node
# is kept, or a graph has one node, the gap is infinite and the seed is 1.
TRUNK_CASES = [
    ("n200-h1000-d4-o1-mask-r0.8", "n200", 1000, 4, 1, True, 0.8, 410),  # searched 1..410
    ("n200-h1000-d4-o100-nomask-r0.8", "n200", 1000, 4, 100, False, 0.8, 368),  # searched 1..368
    ("mixed-h8-d4-o1-mask-r0.5", "mixed", 8, 4, 1, True, 0.5, 349),  # searched 1..349
    ("batch-h1000-d2-o1-mask-r1", "batch", 1000, 2, 1, True, 1.0, 1),
    ("n130-h1000-d2-o100-nomask-r1", "n130", 1000, 2, 100, False, 1.0, 1),
    ("single-h1000-d4-o1-nomask-r0.5", "single", 1000, 4, 1, False, 0.5, 1),
    ("two-h1000-d4-o1-mask-r0.5", "two", 1000, 4, 1, True, 0.5, 1),
    ("fan-h1000-d4-o100-mask-r0.5", "fan", 1000, 4, 100, True, 0.5, 1),
]
TRUNK_IDS = [c[0] for c in TRUNK_CASES]
MODULE_SEED = 1  # GraphUNet(5, 1000, 1000, 4) on the module batch of tests/test_gpu_unet.py: searched 1..1


def trunk_case(kind, hidden, depth, out_dim, with_mask, ratio, seed):
    """(model, x, edge_index, edge_attr, sizes, mask, d_out): the restatement with random weights and the inputs, all from the seed."""
    gen = _gen("trunk", kind, hidden, depth, out_dim, seed)
    torch.manual_seed(100 * seed + hidden + depth + out_dim)
    model = unet_ref.RefGraphUNet(5, hidden, depth, ratio, out_dim)
    with torch.no_grad():
        # GCNConv's biases start at zero: give them values that matter, a down conv's at its level's scale (every gate multiplies the
        # activations by |s| ~ 0.1; a larger bias would be all a deep level's scores see)
        for k, p in model.named_parameters():
            if k.endswith("bias") and "conv" in k:
                scale = 0.05 * 0.1 ** int(k.split(".")[1]) if k.startswith("down") else 0.05
                p.uniform_(-scale, scale)
    n, ei, ea, sizes = trunk_graph(kind, gen)
    x = torch.randn(n, 5, generator=gen)
    x[:, 4] = torch.randint(-1, 2, (n,), generator=gen).float()
    mask = (torch.rand(n, hidden, generator=gen) >= 0.5).float() * 2.0 if with_mask else None
    d_out = torch.randn(n, out_dim, generator=gen)
    return model, x, ei, ea, sizes, mask, d_out
