"""Plain-torch restatement of the g-U-Net networks (scripts/Networks.py:125-449 over PyG 1.x GraphUNet / TopKPooling / GCNConv): the
checker of tests/test_unet_cpu.py and tests/test_gpu_unet.py.  CPU, float64 or float32 (`.double()` / `.float()` on the module).

    x_0 = relu(conv_d0(x, A_0))
    l = 1..depth:  B = offdiag((A_{l-1} + I)^2),  s = tanh(x_{l-1} . p_l / |p_l|),  perm_l = per graph the ceil(ratio n_g) nodes of
                   largest s,  A_l = B[perm_l, perm_l] relabelled,  x_l = relu(conv_dl(x_{l-1}[perm_l] * s[perm_l], A_l))
    i = 0..depth-1, j = depth-1-i:  up = 0, up[perm_{j+1}] = x,  x = conv_ui(x_j + up, A_j), relu except after the last
    out = fully_con1(relu(x) * dropout_mask)

M[edge_index[0][e], edge_index[1][e]] = edge_attr[e], duplicates sum.  The augment is a DENSE product per graph; B keeps every
structurally non-zero off-diagonal entry.  The selection ranks by counting (no torch.topk): node j beats node i with a larger
score, or with the same score and a lower index; kept nodes stay in ascending index.  GCNConv(improved=True): self loop 2 (an
explicit self loop keeps its own weight), deg = row sum, deg^-1/2[row] w deg^-1/2[col], aggregation at the column node.
`state_dict` keys as the reference's classes: down_convs.N.{weight,bias}, pools.N.weight, up_convs.N.{weight,bias},
fully_con1.{weight,bias}."""
import math

import torch


def keep_count(n, ratio):
    """ceil(ratio n) of the double product, at least one node, at most all."""
    return 0 if n <= 0 else max(1, min(n, int(math.ceil(ratio * n))))


def level_sizes(sizes, ratio, depth):
    out = [list(sizes)]
    for _ in range(depth):
        out.append([keep_count(n, ratio) for n in out[-1]])
    return out


def select(scores, sizes, ratio):
    """Per graph the kept nodes (global ids, ascending) by rank counting, and the gap between the k-th and the (k+1)-th score of
    every graph (inf where every node is kept)."""
    perm, gaps, off = [], [], 0
    for n in sizes:
        s = scores[off:off + n]
        k = keep_count(n, ratio)
        idx = torch.arange(n)
        beats = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (idx[None, :] < idx[:, None]))
        rank = beats.sum(1)
        perm.append(off + torch.nonzero(rank < k).view(-1))
        if 0 < k < n:
            by_rank = torch.empty(n, dtype=s.dtype)
            by_rank[rank] = s
            gaps.append(float(by_rank[k - 1] - by_rank[k]))
        else:
            gaps.append(math.inf)
        off += n
    return (torch.cat(perm) if perm else torch.zeros(0, dtype=torch.long)), gaps


def augment_filter(edge_index, edge_attr, sizes, perm, new_sizes):
    """offdiag((A + I)^2) of every graph as a dense product, restricted to the kept nodes and relabelled to pooled ids.
    Returns (edge_index [2, E'], edge_attr [E'], entries per graph), entries sorted by (row, column) inside a graph."""
    eis, ews, counts, off, noff = [], [], [], 0, 0
    for n, k in zip(sizes, new_sizes):
        sel = (edge_index[0] >= off) & (edge_index[0] < off + n) & (edge_index[1] >= off) & (edge_index[1] < off + n)
        r, c, w = edge_index[0][sel] - off, edge_index[1][sel] - off, edge_attr[sel]
        eye = torch.eye(n, dtype=edge_attr.dtype)
        M = torch.zeros(n, n, dtype=edge_attr.dtype).index_put_((r, c), w, accumulate=True) + eye
        P = torch.zeros(n, n, dtype=torch.float64).index_put_((r, c), torch.ones(r.numel(), dtype=torch.float64)) + torch.eye(n, dtype=torch.float64)
        B, PB = M @ M, (P @ P) > 0
        kept = perm[noff:noff + k] - off
        sub, pat = B[kept][:, kept], PB[kept][:, kept] & ~torch.eye(k, dtype=torch.bool)
        rc = torch.nonzero(pat)
        eis.append(rc.t() + noff)
        ews.append(sub[rc[:, 0], rc[:, 1]])
        counts.append(rc.shape[0])
        off += n
        noff += k
    return torch.cat(eis, 1), torch.cat(ews), counts


def augment_rows_sparse(edge_index, edge_attr, sizes, perm, new_sizes):
    """The same rule as `augment_filter` without a dense matrix, in plain Python over rows of dictionaries: per graph the list of
    (kept local node i, {local column j: ((A + I)^2)[i][j]}) for the KEPT rows only, every structurally non-zero column (the diagonal
    and dropped columns included).  M[i] = {j: summed weight} with the 1 of the identity added on the diagonal; a key is structure,
    whatever its value.  Cost: the edges once, then per kept row its neighbours' rows."""
    src, dst, w = edge_index[0].tolist(), edge_index[1].tolist(), edge_attr.tolist()
    perm = perm.tolist()
    graphs, off, noff = [], 0, 0
    for n, k in zip(sizes, new_sizes):
        M = {}
        for a, b, v in zip(src, dst, w):
            if off <= a < off + n and off <= b < off + n:
                row = M.setdefault(a - off, {})
                row[b - off] = row.get(b - off, 0.0) + v
        rows = []
        for i in (p - off for p in perm[noff:noff + k]):
            left = dict(M.get(i, {}))
            left[i] = left.get(i, 0.0) + 1.0
            acc = {}
            for m, v in left.items():
                right = dict(M.get(m, {}))
                right[m] = right.get(m, 0.0) + 1.0
                for j, u in right.items():
                    acc[j] = acc.get(j, 0.0) + v * u
            rows.append((i, acc))
        graphs.append(rows)
        off += n
        noff += k
    return graphs


def augment_filter_sparse(edge_index, edge_attr, sizes, perm, new_sizes):
    """`augment_filter` from `augment_rows_sparse`: the same three results, for graphs too large for the dense product."""
    graphs = augment_rows_sparse(edge_index, edge_attr, sizes, perm, new_sizes)
    perm = perm.tolist()
    r, c, ws, counts, off, noff = [], [], [], [], 0, 0
    for n, k, rows in zip(sizes, new_sizes, graphs):
        new = {p - off: noff + m for m, p in enumerate(perm[noff:noff + k])}
        before = len(r)
        for i, acc in rows:
            for j in sorted(acc):
                if j != i and j in new:
                    r.append(new[i])
                    c.append(new[j])
                    ws.append(acc[j])
        counts.append(len(r) - before)
        off += n
        noff += k
    return torch.tensor([r, c], dtype=torch.long).view(2, -1), torch.tensor(ws, dtype=edge_attr.dtype), counts


class GCNConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        stdv = math.sqrt(6.0 / (in_channels + out_channels))
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)

    def forward(self, x, edge_index, edge_weight):
        n = x.shape[0]
        loop = edge_index[0] == edge_index[1]
        self_w = torch.full((n,), 2.0, dtype=x.dtype)
        self_w[edge_index[0][loop]] = edge_weight[loop]
        row = torch.cat([edge_index[0][~loop], torch.arange(n)])
        col = torch.cat([edge_index[1][~loop], torch.arange(n)])
        w = torch.cat([edge_weight[~loop], self_w])
        deg = torch.zeros(n, dtype=x.dtype).index_add_(0, row, w)
        dis = deg.pow(-0.5)
        dis[torch.isinf(dis)] = 0
        norm = dis[row] * w * dis[col]
        h = x @ self.weight
        return torch.zeros_like(h).index_add_(0, col, norm.unsqueeze(1) * h[row]) + self.bias


class TopKPooling(torch.nn.Module):
    def __init__(self, in_channels, ratio=0.5):
        super().__init__()
        self.ratio = ratio
        self.weight = torch.nn.Parameter(torch.empty(1, in_channels))
        bound = 1.0 / math.sqrt(in_channels)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)

    def score(self, x):
        return torch.tanh((x * self.weight).sum(dim=-1) / self.weight.norm(p=2, dim=-1))


class RefGraphUNet(torch.nn.Module):
    """The trunk shared by GraphUNet (out_dim 1), PolicyGraphUNet (1) and ValueGraphUNet (100).  `mask`: the dropout mask (0 or
    1 / (1 - p)) that F.dropout would have applied, or None; `sizes`: node counts of the batch's graphs (None: one graph).
    After a forward `self.levels` holds per level the scores, the kept nodes, the score gaps per graph and the largest |score|."""

    def __init__(self, in_channels=5, hidden=1000, depth=3, ratio=0.5, out_dim=1):
        super().__init__()
        self.depth, self.ratio = depth, ratio
        self.down_convs = torch.nn.ModuleList([GCNConv(in_channels, hidden)])
        self.pools = torch.nn.ModuleList()
        for _ in range(depth):
            self.pools.append(TopKPooling(hidden, ratio))
            self.down_convs.append(GCNConv(hidden, hidden))
        self.up_convs = torch.nn.ModuleList([GCNConv(hidden, hidden) for _ in range(depth)])
        self.fully_con1 = torch.nn.Linear(hidden, out_dim)

    def trunk_parameters(self):
        return tuple(self.parameters())

    def forward(self, x, edge_index, edge_attr, mask=None, sizes=None):
        sizes = [x.shape[0]] if sizes is None else list(sizes)
        edge_attr = edge_attr.detach()  # edge weights are data
        x = torch.relu(self.down_convs[0](x, edge_index, edge_attr))
        xs, graphs, perms = [x], [(edge_index, edge_attr)], []
        self.levels = []
        for l in range(1, self.depth + 1):
            s = self.pools[l - 1].score(x)
            perm, gaps = select(s.detach(), sizes, self.ratio)
            new_sizes = [keep_count(n, self.ratio) for n in sizes]
            edge_index, edge_attr, _ = augment_filter(edge_index, edge_attr, sizes, perm, new_sizes)
            self.levels.append({"scores": s.detach(), "perm": perm, "gaps": gaps, "max_abs": float(s.detach().abs().max()), "sizes": new_sizes})
            x = torch.relu(self.down_convs[l](x[perm] * s[perm].unsqueeze(1), edge_index, edge_attr))
            sizes = new_sizes
            if l < self.depth:
                xs.append(x)
                graphs.append((edge_index, edge_attr))
            perms.append(perm)
        for i in range(self.depth):
            j = self.depth - 1 - i
            up = torch.zeros_like(xs[j])
            up[perms[j]] = x
            x = self.up_convs[i](xs[j] + up, *graphs[j])
            if i < self.depth - 1:
                x = torch.relu(x)
        x = torch.relu(x)
        if mask is not None:
            x = x * mask
        return self.fully_con1(x)


def policy_head(q, sel, batch, n_graphs):
    """PolicyGraphUNet: masked_select + torch_geometric.utils.softmax over the ORIGINAL batch vector."""
    q, b = q.view(-1)[sel], batch[sel]
    mx = torch.full((n_graphs,), -float("inf"), dtype=q.dtype).scatter_reduce(0, b, q, reduce="amax", include_self=True)
    e = (q - mx[b]).exp()
    return e / (torch.zeros(n_graphs, dtype=q.dtype).index_add_(0, b, e)[b] + 1e-16)


def value_head(h, batch, n_graphs):
    """ValueGraphUNet: global_mean_pool(h, batch).mean(dim=1)."""
    s = torch.zeros(n_graphs, h.shape[1], dtype=h.dtype).index_add_(0, batch, h)
    cnt = torch.zeros(n_graphs, dtype=h.dtype).index_add_(0, batch, torch.ones_like(batch, dtype=h.dtype))
    return (s / cnt.unsqueeze(1)).mean(dim=1)
