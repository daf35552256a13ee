"""Test-side checker of the batched graph export (Engine.graph / drlgx_graph) against the oracle's restatement of
ExplorationEnv.graph_matrix + DeepQ.data_process: topology, edge order, frontier cells and the type column exact, the other
features and the edge weights to float32 round-off.  Shared by test_gpu_graph.py and test_gpu_graph_edges.py."""
import ctypes as C

import numpy as np
import torch

from oracle import oracle as O

_HOST_KEYS = ("node_off", "edge_off", "x", "edge_index", "edge_attr", "n_frontier", "frontier_xy", "nearest_frontier_node", "batch")


def oracle_graph(env):
    """What one OracleEnv exports now: a dict to compare any number of engine slices with (the env's frontier state is updated as
    graph_matrix does)."""
    A, X, _, fro = env.graph_matrix()
    ei, ea, x = O.data_process(A, X)
    return dict(N=A.shape[0], F=fro, x=x, edge_index=ei, edge_attr=ea, frontier_xy=np.array(env._frontier, dtype=np.float64).reshape(-1, 2),
                nearest=env.nearest_frontier_point)


def graph_to_host(g):
    """The export's tensors as numpy arrays (arrays pass through)."""
    return {k: (g[k].cpu().numpy() if isinstance(g[k], torch.Tensor) else np.asarray(g[k])) for k in _HOST_KEYS if k in g}


def check_graph_slice(h, i, og):
    """Slice `i` of the host copy `h` (graph_to_host) of a batched export equals the oracle graph `og` (oracle_graph)."""
    node_off, edge_off = h["node_off"], h["edge_off"]
    N, fro = og["N"], og["F"]
    assert node_off[i + 1] - node_off[i] == N
    assert h["n_frontier"][i] == fro
    np.testing.assert_array_equal(h["frontier_xy"][i, :fro], og["frontier_xy"])
    assert h["nearest_frontier_node"][i] == og["nearest"]
    xs = h["x"][node_off[i]:node_off[i + 1]]
    # features are float32 casts of float64 values computed the same way
    np.testing.assert_allclose(xs, og["x"], rtol=2e-6, atol=1e-7)
    assert np.all(xs[:, 4] == og["x"][:, 4])
    E = og["edge_index"].shape[1]
    assert edge_off[i + 1] - edge_off[i] == E
    es = h["edge_index"][:, edge_off[i]:edge_off[i + 1]] - node_off[i]
    np.testing.assert_array_equal(es, og["edge_index"])  # topology and edge order exact
    np.testing.assert_allclose(h["edge_attr"][edge_off[i]:edge_off[i + 1]], og["edge_attr"], rtol=1e-6)
    if "batch" in h:
        assert np.all(h["batch"][node_off[i]:node_off[i + 1]] == i)
    return N, fro


def check_graphs(eng, envs, g, skip=()):
    """Every env's slice of the export `g` against its OracleEnv (`skip`: env ids left out); returns [(nodes, frontiers)]."""
    h = graph_to_host(g)
    out = []
    for i, env in enumerate(envs):
        if i in skip:
            out.append((int(h["node_off"][i + 1] - h["node_off"][i]), int(h["n_frontier"][i])))
            continue
        out.append(check_graph_slice(h, i, oracle_graph(env)))
    return out


X_SENTINEL = -12345.0      # no feature, weight or coordinate takes these values
INDEX_SENTINEL = -7777


def raw_graph(eng):
    """One drlgx_graph call through the C ABI into buffers of graph_capacity() size prefilled with sentinels.  Asserts that nothing
    was written past what the export reports - x beyond node_off[n] rows, edge_attr beyond edge_off[n], edge_index beyond its two
    rows, which lie at offsets 0 and edge_off[n] (NOT at the capacity), frontier_xy beyond n_frontier[i] - and returns
    (host dict as graph_to_host gives it, without `batch`; the device status word read after the call)."""
    eng.use_torch_stream()
    mn, me, mf = eng.graph_capacity()
    n, dev = eng.n_envs, eng.device
    node_off = torch.full((n + 1,), INDEX_SENTINEL, dtype=torch.int32, device=dev)
    edge_off = torch.full((n + 1,), INDEX_SENTINEL, dtype=torch.int32, device=dev)
    x = torch.full((mn, 5), X_SENTINEL, dtype=torch.float32, device=dev)
    ei = torch.full((2 * me,), INDEX_SENTINEL, dtype=torch.int64, device=dev)
    ea = torch.full((me,), X_SENTINEL, dtype=torch.float32, device=dev)
    nfr = torch.full((n,), INDEX_SENTINEL, dtype=torch.int32, device=dev)
    fxy = torch.full((n, mf, 2), X_SENTINEL, dtype=torch.float64, device=dev)
    near = torch.full((n,), INDEX_SENTINEL, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = eng.L.drlgx_graph(eng.h, p(node_off), p(edge_off), p(x), p(ei), p(ea), p(nfr), p(fxy), p(near))
    assert rc == 0, rc
    status = eng.status()  # (synchronises)
    node_off, edge_off, x, ei, ea, nfr, fxy, near = (t.cpu().numpy() for t in (node_off, edge_off, x, ei, ea, nfr, fxy, near))
    N, E = int(node_off[n]), int(edge_off[n])
    assert node_off[0] == 0 and edge_off[0] == 0 and 0 <= N <= mn and 0 <= E <= me
    assert np.all(np.diff(node_off) >= 0) and np.all(np.diff(edge_off) >= 0)
    assert np.all(x[N:] == X_SENTINEL), "x written beyond node_off[n] rows"
    assert np.all(x[:N] != X_SENTINEL), "a row of x below node_off[n] not (fully) written"
    assert np.all(ea[E:] == X_SENTINEL), "edge_attr written beyond edge_off[n]"
    assert np.all(ea[:E] != X_SENTINEL), "an edge weight below edge_off[n] not written"
    assert np.all(ei[2 * E:] == INDEX_SENTINEL), "edge_index written beyond its two rows of edge_off[n] entries"
    assert np.all(ei[:2 * E] != INDEX_SENTINEL), "edge_index: row 1 does not start at offset edge_off[n]"
    assert np.all((nfr >= 0) & (nfr <= mf)) and np.all(near != INDEX_SENTINEL)
    for i in range(n):
        assert np.all(fxy[i, nfr[i]:] == X_SENTINEL), "frontier_xy written beyond n_frontier"
        assert np.all(fxy[i, :nfr[i]] != X_SENTINEL)
    h = dict(node_off=node_off, edge_off=edge_off, x=x[:N], edge_index=ei[:2 * E].reshape(2, E), edge_attr=ea[:E], n_frontier=nfr,
             frontier_xy=fxy, nearest_frontier_node=near)
    # the two rows are each other's mirror, pair by pair: (i, j) then (j, i)
    assert np.array_equal(h["edge_index"][0, 0::2], h["edge_index"][1, 1::2]) and np.array_equal(h["edge_index"][0, 1::2], h["edge_index"][1, 0::2])
    return h, status
