"""Plain-torch restatement of the GG-NN networks (scripts/Networks.py:73-122 over PyG 1.x GatedGraphConv(1000, 3)): the checker
of tests/test_ggnn_cpu.py and tests/test_gpu_ggnn.py.  CPU, float64 or float32 (`.double()` / `.float()` on the module).

    h_0 = [x | 0];  per layer  m = h @ weight[l],  a[i] = sum over edges e into i of edge_attr[e] m[edge_index[0][e]],
    h = GRUCell(a, h);  out = fully_con1(relu(h) * dropout_mask)

The aggregation is `index_add_` at the TARGET node, the products `torch.nn.functional.linear`, the cell a real
`torch.nn.GRUCell`.  `state_dict` keys as the reference's classes: gconv1.weight, gconv1.rnn.{weight,bias}_{ih,hh},
fully_con1.{weight,bias}.

`dense=True` is a second restatement of the aggregation alone, independent of `index_add_`: the adjacency as a dense matrix,
A[dst, src] += w (`index_put_` with accumulate: repeated edges add up, an explicit self loop is a diagonal entry), and
a = A @ (h @ weight[l]).  tests/test_ggnn_cpu.py holds the two against each other in float64."""
import math

import torch


class GatedGraphConv(torch.nn.Module):
    def __init__(self, out_channels, num_layers, dense=False):
        super().__init__()
        self.out_channels, self.num_layers, self.dense = out_channels, num_layers, dense
        self.weight = torch.nn.Parameter(torch.empty(num_layers, out_channels, out_channels))
        self.rnn = torch.nn.GRUCell(out_channels, out_channels)
        bound = 1.0 / math.sqrt(out_channels)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)

    def forward(self, x, edge_index, edge_weight):
        h = torch.cat([x, x.new_zeros(x.shape[0], self.out_channels - x.shape[1])], dim=1)
        if self.dense:
            A = x.new_zeros(x.shape[0], x.shape[0]).index_put_((edge_index[1], edge_index[0]), edge_weight, accumulate=True)
        for l in range(self.num_layers):
            m = torch.nn.functional.linear(h, self.weight[l].t())  # h @ weight[l]
            if self.dense:
                a = A @ m
            else:
                a = torch.zeros_like(m).index_add_(0, edge_index[1], edge_weight.unsqueeze(1) * m[edge_index[0]])
            h = self.rnn(a, h)
        return h


class RefGGNN(torch.nn.Module):
    """The trunk shared by GGNN (out_dim 1), PolicyGGNN (1) and ValueGGNN (100); `mask`: the dropout mask (0 or 1 / (1 - p)) that
    F.dropout would have applied, or None."""

    def __init__(self, hidden=1000, num_layers=3, out_dim=1, dense=False):
        super().__init__()
        self.gconv1 = GatedGraphConv(hidden, num_layers, dense)
        self.fully_con1 = torch.nn.Linear(hidden, out_dim)

    def forward(self, x, edge_index, edge_attr, mask=None):
        return self.read_out(self.gconv1(x, edge_index, edge_attr), mask)

    def read_out(self, h_last, mask=None):
        """From h_L (what `gconv1` returns, before the relu) on: relu, the mask, the linear layer."""
        h = torch.relu(h_last)
        if mask is not None:
            h = h * mask
        return self.fully_con1(h)

    def trunk_parameters(self):
        r = self.gconv1.rnn
        return (self.gconv1.weight, r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh, self.fully_con1.weight, self.fully_con1.bias)


def policy_head(q, sel, batch, n_graphs):
    """PolicyGGNN: masked_select + torch_geometric.utils.softmax (PyG 1.x: exp(q - segment max) / (segment sum + 1e-16))."""
    q, b = q.view(-1)[sel], batch[sel]
    mx = torch.full((n_graphs,), -float("inf"), dtype=q.dtype).scatter_reduce(0, b, q, reduce="amax", include_self=True)
    e = (q - mx[b]).exp()
    return e / (torch.zeros(n_graphs, dtype=q.dtype).index_add_(0, b, e)[b] + 1e-16)


def value_head(h, batch, n_graphs):
    """ValueGGNN: global_mean_pool(h, batch).mean(dim=1)."""
    s = torch.zeros(n_graphs, h.shape[1], dtype=h.dtype).index_add_(0, batch, h)
    cnt = torch.zeros(n_graphs, dtype=h.dtype).index_add_(0, batch, torch.ones_like(batch, dtype=h.dtype))
    return (s / cnt.unsqueeze(1)).mean(dim=1)
