"""GPU numerics tests of the HIP GCN kernels (CSR aggregation + fp32-MFMA GEMMs, forward and backward)
against the plain-PyTorch fp32 reference of the same op (oracle/gcn_ref.py, PyG-1.x GCNConv(improved=True)).
Tolerance: 2e-4 of the output scale (fp32; the summation order differs: CSR rows vs index_add_, 1000-long MFMA
dot products vs rocBLAS)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gcn_ref  # noqa: E402  (checker only)


def random_batch(n_graphs, seed, dev, nmin=20, nmax=70):
    g = torch.Generator().manual_seed(seed)
    xs, eis, eas, bs = [], [], [], []
    off = 0
    for k in range(n_graphs):
        n = int(torch.randint(nmin, nmax, (1,), generator=g))
        m = int(torch.randint(n, 3 * n, (1,), generator=g))
        src = torch.randint(0, n, (m,), generator=g)
        dst = torch.randint(0, n, (m,), generator=g)
        keep = src != dst
        src, dst = src[keep], dst[keep]
        w = torch.rand(src.shape[0], generator=g) * 5.9 + 0.1
        # symmetric, both directions like data_process
        ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])]) + off
        ea = torch.cat([w, w])
        x = torch.randn(n, 5, generator=g)
        x[:, 4] = torch.randint(-1, 2, (n,), generator=g).float()
        xs.append(x); eis.append(ei); eas.append(ea); bs.append(torch.full((n,), k, dtype=torch.long))
        off += n
    return (torch.cat(xs).to(dev), torch.cat(eis, 1).to(dev), torch.cat(eas).to(dev), torch.cat(bs).to(dev))


def make_params(dev, out_dim=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = {
        "conv1.weight": torch.randn(5, 1000, generator=g) * 0.08, "conv1.bias": torch.randn(1000, generator=g) * 0.05,
        "conv2.weight": torch.randn(1000, 1000, generator=g) * 0.03, "conv2.bias": torch.randn(1000, generator=g) * 0.05,
        "fully_con1.weight": torch.randn(out_dim, 1000, generator=g) * 0.03, "fully_con1.bias": torch.randn(out_dim, generator=g) * 0.05,
    }
    return {k: v.to(dev).requires_grad_(True) for k, v in p.items()}


def batch_of_about(n_nodes, seed, dev):
    """A random batch whose node count is n_nodes (graphs of 20..69 nodes; the last one trimmed to fit by regenerating)."""
    g = torch.Generator().manual_seed(seed)
    sizes = []
    while sum(sizes) < n_nodes:
        sizes.append(int(torch.randint(20, 70, (1,), generator=g)))
    sizes[-1] -= sum(sizes) - n_nodes
    if sizes[-1] < 2:
        sizes[-2] += sizes.pop()
    xs, eis, eas = [], [], []
    off = 0
    for n in sizes:
        m = int(torch.randint(n, 3 * n, (1,), generator=g))
        src, dst = torch.randint(0, n, (m,), generator=g), torch.randint(0, n, (m,), generator=g)
        keep = src != dst
        src, dst = src[keep], dst[keep]
        w = torch.rand(src.shape[0], generator=g) * 5.9 + 0.1
        eis.append(torch.stack([torch.cat([src, dst]), torch.cat([dst, src])]) + off)
        eas.append(torch.cat([w, w]))
        x = torch.randn(n, 5, generator=g)
        x[:, 4] = torch.randint(-1, 2, (n,), generator=g).float()
        xs.append(x)
        off += n
    return torch.cat(xs).to(dev), torch.cat(eis, 1).to(dev), torch.cat(eas).to(dev)


def rel_err(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_tall_tile_gemm_heights_are_all_exercised():
    """The batches of the parametrised test below make the dispatcher pick every compiled tile of the tall-tile GEMM
    (k_gemm_wide) for the forward / dZ2 W2^T products - five heights of the 8-wave kernel (128 columns), three of the 4-wave
    one (64 columns) - and the 128 x 128 one for the split-K weight gradient (asked of the library itself, as 1000 * columns +
    rows, so the test cannot drift from the dispatch rule)."""
    from drl_graph_exploration_amd import _lib
    L = _lib.lib()
    picked = {L.drlgx_debug_gemm_tile_rows(n, 1000, 1, 0) for n in TALL_TILE_NODES}
    assert picked == {128096, 128112, 128128, 128144, 128160, 64096, 64112, 64128}, picked
    assert L.drlgx_debug_gemm_tile_rows(1000, 1000, 4, 1) == 128128
    assert L.drlgx_debug_gemm_tile_rows(900, 1000, 1, 0) == 64064  # (small batches stay on the 64x64 kernels)


# node counts (odd ones too: ragged last row tile) per tile: 96 .. 128 x 64 (4 waves), 96 .. 160 x 128 (8 waves)
TALL_TILE_NODES = (1101, 1700, 1903, 3050, 3301, 3803, 4342, 4799)


@pytest.mark.parametrize("n_graphs,out_dim,with_mask", [(1, 1, False), (7, 1, True), (64, 1, False), (5, 100, True), (9, 3, True), (6, 8, False)] +
                         [(-n, 1, n % 2 == 0) for n in TALL_TILE_NODES] +
                         # (seeded instances: about one 12.8 k-node batch in four has a ReLU pre-activation within fp32 round-off of 0 whose
                         # gate flips in ours or in torch's fp32 evaluation - 1e-4 .. 1e-3 of the gradient norm either way, for every read-out
                         # width, scripts/gcn_grad_errors.py; 12 807 is one without)
                         # the critic's 100-wide read-out (and a width that is no multiple of 4: the unvectorised kernels) on the matrix
                         # cores: 64 x 64 tiles, the 4-wave and the 8-wave tall tiles for its forward / dZ2 products
                         [(40, 100, True), (-1903, 100, False), (-4799, 100, True), (-12807, 100, True), (-1700, 10, True)])
def test_gcn_forward_backward_matches_torch_reference(n_graphs, out_dim, with_mask):
    from drl_graph_exploration_amd.networks import gcn_trunk
    dev = torch.device("cuda", 0)
    if n_graphs > 0:
        x, ei, ea, batch = random_batch(n_graphs, 123 + n_graphs, dev)
    else:  # a batch of exactly -n_graphs nodes (the tall-tile GEMM path)
        x, ei, ea = batch_of_about(-n_graphs, 77 - n_graphs, dev)
    P = make_params(dev, out_dim)
    N = x.shape[0]
    mask = None
    if with_mask:
        mask = (torch.rand(N, 1000, device=dev, generator=torch.Generator(device=dev).manual_seed(11 + N)) >= 0.5).float() * 2.0
    out = gcn_trunk(x, ei, ea, P["conv1.weight"], P["conv1.bias"], P["conv2.weight"], P["conv2.bias"], P["fully_con1.weight"],
                    P["fully_con1.bias"], mask)
    # the same plain-torch reference evaluated in float64 is the ground truth (in float32 a ReLU gate that sits at
    # ~0 can flip inside the reference itself and move a gradient by 1e-4); the float32 evaluation is checked too
    ref_params = {k: v.detach().double().clone().requires_grad_(True) for k, v in P.items()}
    ref = gcn_ref.gcn_forward(ref_params, x.double(), ei, ea.double(), None if mask is None else mask.double())
    assert out.shape == ref.shape == (N, out_dim)
    assert rel_err(out.detach().double(), ref.detach()) < 1e-5
    with torch.no_grad():
        ref32 = gcn_ref.gcn_forward({k: v.detach() for k, v in P.items()}, x, ei, ea, mask)
    assert rel_err(out.detach(), ref32) < 2e-4
    # backward with a DQN-style weighted sum over the node outputs
    wgt = torch.randn(N, out_dim, device=dev, generator=torch.Generator(device=dev).manual_seed(3 + N))
    (out * wgt).sum().backward()
    (ref * wgt.double()).sum().backward()
    # the same plain-torch reference in float32, to calibrate what fp32 round-off does to this problem
    p32 = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    (gcn_ref.gcn_forward(p32, x, ei, ea, mask) * wgt).sum().backward()
    for k in P:
        assert P[k].grad is not None, k
        # typical agreement is ~1e-6; a ReLU pre-activation within fp32 round-off of 0 flips its gate in ANY fp32
        # evaluation (here or in torch) and moves single gradient entries by up to ~1e-3 of the max: bound the
        # max-norm loosely, and the Frobenius norm by what the plain fp32 torch evaluation itself achieves against
        # the float64 ground truth (x3), with 1e-4 as the floor
        g, r = P[k].grad.double(), ref_params[k].grad
        e_ours = float((g - r).norm() / r.norm())
        e_torch32 = float((p32[k].grad.double() - r).norm() / r.norm())
        m_ours, m_torch32 = rel_err(g, r), rel_err(p32[k].grad.double(), r)
        assert m_ours < max(2e-3, 3.0 * m_torch32), (k, m_ours, m_torch32)
        assert e_ours < max(1e-4, 3.0 * e_torch32), (k, e_ours, e_torch32)


def test_reference_state_dict_loads_and_picks_reference_actions(golden_dir):
    """The shipped DQN_GCN/MyModel.pt loads into GCN() unchanged and the HIP forward (dropout p = 0, as test.py)
    reproduces the plain-torch forward on a real exploration graph batch."""
    from drl_graph_exploration_amd.networks import GCN, GraphData
    dev = torch.device("cuda", 0)
    sd = torch.load(os.path.join(golden_dir, "DQN_GCN_MyModel.pt"), map_location="cpu")
    model = GCN()
    model.load_state_dict(sd)  # same keys and shapes as the reference's Networks.GCN
    model.to(dev)
    x, ei, ea, batch = random_batch(16, 7, dev)
    x[:, 0] = x[:, 0].abs() * 0.05  # trace-like feature
    x[:, 1] = x[:, 1].abs() * 8
    x[:, 2] = x[:, 2].abs()
    x[:, 3] = 0.3
    data = GraphData(x, ei, ea, batch)
    with torch.no_grad():
        q = model(data, 0.0, batch=batch)
        ref = gcn_ref.gcn_forward({k: v.to(dev) for k, v in sd.items()}, x, ei, ea)
    assert rel_err(q, ref) < 2e-4
    # per-graph argmax (the action choice) agrees
    for g in range(16):
        m = batch == g
        assert int(q[m].argmax()) == int(ref[m].argmax())


def test_policy_and_value_heads():
    from drl_graph_exploration_amd.networks import PolicyGCN, ValueGCN, GraphData
    dev = torch.device("cuda", 0)
    x, ei, ea, batch = random_batch(6, 99, dev)
    data = GraphData(x, ei, ea, batch)
    torch.manual_seed(0)
    pol = PolicyGCN().to(dev)
    val = ValueGCN().to(dev)
    sel = (x[:, 4] > 0)
    for g in range(6):  # make sure every graph has a candidate
        idx = int((batch == g).nonzero()[0])
        sel[idx] = True
    probs = pol(data, sel, batch=batch)
    assert probs.shape[0] == int(sel.sum())
    sums = torch.zeros(6, device=dev).index_add_(0, batch[sel], probs)
    assert torch.allclose(sums, torch.ones(6, device=dev), atol=1e-5)
    v = val(data, sel, batch=batch)
    assert v.shape == (6,)
    (probs.log().sum() + v.sum()).backward()
    for p in list(pol.parameters()) + list(val.parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all()


def test_a2c_heads_and_losses_match_torch_reference(monkeypatch, tmp_path):
    """PolicyGCN / ValueGCN (Networks.py:31-70) and the A2C losses (policy.py:452-497) through the HIP trunk, against the
    plain-torch float64 restatement with the same (fixed) dropout mask: head outputs and the gradients of the combined
    loss with respect to every parameter of both networks."""
    import drl_graph_exploration_amd.networks as NW
    from drl_graph_exploration_amd.networks import PolicyGCN, ValueGCN, GraphData
    from drl_graph_exploration_amd.policy import A2C
    dev = torch.device("cuda", 0)
    n_graphs = 5
    x, ei, ea, batch = random_batch(n_graphs, 4242, dev)
    N = x.shape[0]
    sel = x[:, 4] > 0
    for g in range(n_graphs):
        sel[int((batch == g).nonzero()[0])] = True  # every graph has a candidate
    torch.manual_seed(3)
    fixed = (torch.rand(N, 1000, device=dev) >= 0.5).float() * 2.0  # F.dropout(x) with p = 0.5, frozen for the comparison
    monkeypatch.setattr(NW, "_dropout_mask", lambda n, hidden, p, device: fixed)
    pol, val = PolicyGCN().to(dev), ValueGCN().to(dev)
    data = GraphData(x, ei, ea, batch)
    a2c = A2C("t/", data_root=str(tmp_path))
    a2c.nstep = n_graphs
    # one chosen frontier node per graph, advantages and returns
    action = torch.zeros(N, device=dev)
    adv = torch.zeros(N, device=dev)
    gsel = torch.Generator().manual_seed(1)
    for g in range(n_graphs):
        idx = (sel & (batch == g)).nonzero().view(-1)
        pick = int(idx[int(torch.randint(0, idx.numel(), (1,), generator=gsel))])
        action[pick] = 1.0
        adv[pick] = float(torch.randn(1, generator=gsel))
    ret = torch.randn(n_graphs, generator=gsel).to(dev)

    def losses(probs, values):
        return a2c.policy_cost(probs + 1e-35, adv.to(probs.dtype), action.to(probs.dtype), sel) \
            - a2c.entropy_loss(probs + 1e-35) * a2c.ent_coef + a2c.value_cost(values, ret.to(values.dtype)) * a2c.vf_coef

    probs, values = pol(data, sel, batch=batch), val(data, sel, batch=batch)
    losses(probs, values).backward()
    # float64 torch reference with the same parameters and mask
    pp = {k: v.detach().double().clone().requires_grad_(True) for k, v in pol.state_dict().items()}
    pv = {k: v.detach().double().clone().requires_grad_(True) for k, v in val.state_dict().items()}
    rprobs = gcn_ref.policy_gcn_forward(pp, x.double(), ei, ea.double(), sel, batch, n_graphs, fixed.double())
    rvalues = gcn_ref.value_gcn_forward(pv, x.double(), ei, ea.double(), batch, n_graphs, fixed.double())
    assert rel_err(probs.double(), rprobs) < 1e-5 and rel_err(values.double(), rvalues) < 1e-5
    sums = torch.zeros(n_graphs, device=dev).index_add_(0, batch[sel], probs.detach())
    assert torch.allclose(sums, torch.ones(n_graphs, device=dev), atol=1e-5)
    losses(rprobs, rvalues).backward()
    for model, ref in ((pol, pp), (val, pv)):
        for k, p in model.named_parameters():
            g, r = p.grad.double(), ref[k].grad
            # (the actor's output bias has an exactly zero gradient - softmax is shift invariant: absolute floor)
            assert float((g - r).norm()) < 2e-4 * float(r.norm()) + 1e-6, k


def test_dqn_minibatch_matches_float64_restatement(monkeypatch, tmp_path):
    """One DQN update (scripts/policy.py:139-178, :234-253) through the product path - target network forward on the HIP
    GCN, `DeepQ.td_targets` (the reference's read-out windows), float64 loss, HIP backward, element-wise clamp, Adam -
    against the same update restated in float64 torch + the oracle's numpy target loop: y_batch, loss and the
    parameters after the optimiser step."""
    import random
    import drl_graph_exploration_amd.networks as NW
    from drl_graph_exploration_amd.networks import GCN, GraphData
    from drl_graph_exploration_amd.policy import DeepQ
    from oracle import dqn_ref
    dev = torch.device("cuda", 0)
    B = 8
    gen = torch.Generator().manual_seed(7)
    trans = []
    for k in range(B):
        x, ei, ea, _ = random_batch(1, 900 + k, dev, nmin=12, nmax=30)
        x1, ei1, ea1, _ = random_batch(1, 1900 + k, dev, nmin=int(x.shape[0]), nmax=int(x.shape[0]) + 6)  # graphs grow
        n, fro, fro1 = int(x.shape[0]), 1 + int(torch.randint(0, 4, (1,), generator=gen)), 1 + int(torch.randint(0, 4, (1,), generator=gen))
        a = n - fro + int(torch.randint(0, fro, (1,), generator=gen))
        trans.append((GraphData(x, ei, ea), a, float(torch.randn(1, generator=gen)), GraphData(x1, ei1, ea1), k % 3 == 0, fro1))
    dq = DeepQ("t/", "GCN", data_root=str(tmp_path))
    dq.BATCH = B
    dq.buffer.extend(trans)
    torch.manual_seed(11)
    pol, tgt = GCN().to(dev), GCN().to(dev)
    with torch.no_grad():
        for m in (pol, tgt):  # biases away from zero so that every parameter sees a gradient
            m.conv1.bias.normal_(0, 0.05); m.conv2.bias.normal_(0, 0.05); m.fully_con1.bias.normal_(0, 0.05)
    p0 = {k: v.detach().double().clone() for k, v in pol.state_dict().items()}
    pt = {k: v.detach().double().clone() for k, v in tgt.state_dict().items()}
    N = sum(t[0].num_nodes for t in trans)
    fixed = (torch.rand(N, 1000, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) >= 0.5).float() * 2.0
    monkeypatch.setattr(NW, "_dropout_mask", lambda n, hidden, p, device: fixed if p > 0 else None)
    monkeypatch.setattr(random, "sample", lambda buf, k: list(buf)[:k])  # the minibatch = the 8 transitions, in order
    captured = {}
    orig_train = dq.train

    def spy(data, action, y, device, model, optimizer):
        captured.update(a=action.clone(), y=y.clone())
        return orig_train(data, action, y, device, model, optimizer)
    dq.train = spy
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    dq._train_minibatch(dev, pol, tgt, opt)
    # ---- float64 restatement
    s_j, s_j1 = GraphData.collate([t[0] for t in trans]), GraphData.collate([t[3] for t in trans])
    q1 = gcn_ref.gcn_forward(pt, s_j1.x.double(), s_j1.edge_index, s_j1.edge_attr.double()).detach().cpu().numpy()
    acts = []
    for t in trans:
        act = np.zeros(t[0].num_nodes)
        act[t[1]] = 1
        acts.append(act)
    a_ref, y_ref = dqn_ref.reference_targets(acts, [t[2] for t in trans], [t[4] for t in trans], [t[5] for t in trans], q1, dq.GAMMA)
    np.testing.assert_array_equal(captured["a"].cpu().numpy(), a_ref)
    np.testing.assert_allclose(captured["y"].cpu().numpy(), y_ref, rtol=0, atol=2e-5)  # fp32 target network vs float64
    pr = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    out = gcn_ref.gcn_forward(pr, s_j.x.double(), s_j.edge_index, s_j.edge_attr.double(), fixed.double()).view(-1)
    y_t, a_t = torch.as_tensor(y_ref, device=dev), torch.as_tensor(a_ref, device=dev)
    loss = torch.pow(out * a_t - y_t, 2).sum() / B
    assert dq.temp_loss == pytest.approx(float(loss.detach()), rel=2e-4)
    loss.backward()
    ref_opt = torch.optim.Adam([pr[k] for k in pr], lr=1e-3)
    for k in pr:
        pr[k].grad.clamp_(-dq.max_grad_norm, dq.max_grad_norm)
    ref_opt.step()
    for k, v in pol.state_dict().items():
        # Adam's first step moves every parameter by lr * sign(grad) (up to eps): compare the step, not just the value
        step, rstep = v.double() - p0[k], pr[k].detach() - p0[k]
        assert float((step - rstep).abs().max()) < 2e-2 * 1e-3 + 1e-9, k


def test_fused_dqn_update_equals_the_framework_path(monkeypatch, tmp_path):
    """The DQN update as `DeepQ.running` issues it - mini-batches collated out of the device replay pool by
    drlgx_replay_collate, the target network's read-out evaluated once per stored export and gathered per mini-batch, TD
    targets by drlgx_dqn_targets, cost + gradient by drlgx_dqn_loss_grad, the trunk called without
    an autograd graph, clamp + Adam in drlgx_adam_step - against the same three updates through the framework path (generic
    collate, tensor-op targets on the host copy, autograd, element-wise clamp, torch.optim.Adam): targets and collated
    batches bit-equal, losses and parameters after every step within float32 round-off of the update."""
    import copy
    import random
    import drl_graph_exploration_amd.networks as NW
    from drl_graph_exploration_amd.networks import GCN, GraphData, PoolRef, ReplayPool
    from drl_graph_exploration_amd.optim import FusedAdam
    from drl_graph_exploration_amd.policy import DeepQ
    dev = torch.device("cuda", 0)
    B, n_exports, n_env = 8, 3, 6
    gen = torch.Generator().manual_seed(3)
    pool = ReplayPool(dev, n_exports + 1, 512, 4096)
    pool_cached = ReplayPool(dev, n_exports + 1, 512, 4096, cache_csr=True)  # the same exports with the per-graph CSR cache
    exports = []
    for k in range(n_exports):  # batched exports like Engine.graph: n_env graphs each, host offsets beside
        x, ei, ea, bt = random_batch(n_env, 300 + k, dev, nmin=10 if k == 0 else 18, nmax=18 if k == 0 else 28)  # graphs grow
        cnt = torch.bincount(bt, minlength=n_env).cpu().numpy()
        node_off = np.concatenate([[0], np.cumsum(cnt)])
        ecnt = torch.bincount(bt[ei[0]], minlength=n_env).cpu().numpy()
        edge_off = np.concatenate([[0], np.cumsum(ecnt)])
        g = {"x": x, "edge_index": ei, "edge_attr": ea, "node_off_h": node_off, "edge_off_h": edge_off}
        exports.append((pool.put(g), g))
        assert pool_cached.put(g) == exports[-1][0] and pool_cached.csr_ok[exports[-1][0]]
    plain, pooled = [], []
    for i in range(2 * B):
        (s0, g0), (s1, g1) = exports[0], exports[1 + i % 2]
        e = i % n_env
        r0, r1 = PoolRef(pool, s0, e), PoolRef(pool, s1, e)
        fro1 = 1 + int(torch.randint(0, 3, (1,), generator=gen))
        a = r0.num_nodes - 1 - int(torch.randint(0, 3, (1,), generator=gen))
        rew, term = float(torch.randn(1, generator=gen)), i % 4 == 0
        pooled.append((r0, a, rew, r1, term, fro1))
        plain.append((GraphData(r0.x.clone(), r0.edge_index.clone(), r0.edge_attr.clone()), a, rew,
                      GraphData(r1.x.clone(), r1.edge_index.clone(), r1.edge_attr.clone()), term, fro1))
    # collation out of the pool = the generic concatenation
    cp, cg = GraphData.collate([t[0] for t in pooled[:B]]), GraphData.collate([t[0] for t in plain[:B]])
    for a_, b_ in ((cp.x, cg.x), (cp.edge_index, cg.edge_index), (cp.edge_attr, cg.edge_attr), (cp.batch, cg.batch)):
        assert torch.equal(a_, b_)
    torch.manual_seed(5)
    pol_a = GCN().to(dev)
    with torch.no_grad():
        for b_ in (pol_a.conv1.bias, pol_a.conv2.bias, pol_a.fully_con1.bias):
            b_.normal_(0, 0.05)
    pol_b, tgt = copy.deepcopy(pol_a), copy.deepcopy(pol_a)
    pol_c = copy.deepcopy(pol_a)
    masks = {}

    def fixed_mask(n, hidden, p, device):  # the same Bernoulli(0.5) mask for both paths (keyed by the batch size)
        if p <= 0:
            return None
        if n not in masks:
            masks[n] = (torch.rand(n, hidden, device=device, generator=torch.Generator(device=device).manual_seed(n)) >= 0.5).float() * 2.0
        return masks[n]
    monkeypatch.setattr(NW, "_dropout_mask", fixed_mask)
    dq_a, dq_b = DeepQ("a/", "GCN", data_root=str(tmp_path)), DeepQ("b/", "GCN", data_root=str(tmp_path))
    for dq, buf in ((dq_a, pooled), (dq_b, plain)):
        dq.BATCH = B
        dq.buffer.extend(buf)
    order = [[(3 * u + 5 * j) % (2 * B) for j in range(B)] for u in range(3)]
    opt_a = FusedAdam(pol_a.parameters(), lr=1e-3, grad_clamp=dq_a.max_grad_norm)
    opt_b = torch.optim.Adam(pol_b.parameters(), lr=1e-3)
    it = iter(order)
    monkeypatch.setattr(random, "sample", lambda buf, k: [buf[i] for i in next(it)])
    prepared, _ = dq_a._prepare_updates(3, dev, tgt)  # (this also evaluates the target network once per pooled export)
    assert prepared is not None
    it = iter(order)
    spy = {}
    orig = dq_b.train

    def spy_train(data, action, y, device, model, optimizer):
        spy["y"] = y.clone()
        return orig(data, action, y, device, model, optimizer)
    dq_b.train = spy_train
    orig_a = dq_a.train

    def spy_train_a(data, action, y, device, model, optimizer):
        spy["ya"], spy["aa"] = y.clone(), action.clone()
        return orig_a(data, action, y, device, model, optimizer)
    dq_a.train = spy_train_a
    for u in range(3):
        dq_a._train_minibatch(dev, pol_a, tgt, opt_a, prepared[u])
        dq_b._train_minibatch(dev, pol_b, tgt, opt_b)
        assert torch.equal(spy["ya"], spy["y"])  # same read-out, same windows: bit-equal float64 targets
        assert float(spy["aa"].sum()) == B
        assert dq_a.temp_loss == pytest.approx(dq_b.temp_loss, rel=1e-5)
        for (k, va), vb in zip(pol_a.state_dict().items(), pol_b.state_dict().values()):
            # one Adam step moves a parameter by at most ~lr: the two paths must agree to a small fraction of that
            assert float((va - vb).abs().max()) < 2e-2 * 1e-3 * (u + 1), (u, k)
    assert opt_a.step_count == 3
    # the same three updates through the trainer's loop: two host calls per update (drlgx_dqn_prepare,
    # drlgx_dqn_forward_backward) over one arena - the same launches in the same order, so bit-equal parameters and loss
    dq_c = DeepQ("c/", "GCN", data_root=str(tmp_path))
    dq_c.BATCH = B
    dq_c.buffer.extend(pooled)
    opt_c = FusedAdam(pol_c.parameters(), lr=1e-3, grad_clamp=dq_c.max_grad_norm)
    it = iter(order)
    prepared_c, _ = dq_c._prepare_updates(3, dev, tgt)
    calls = []
    orig_fb = dq_c._fused_forward_backward
    dq_c._fused_forward_backward = lambda *a, **k: (calls.append(1), orig_fb(*a, **k))[1]
    dq_c._train_minibatches(dev, pol_c, tgt, opt_c, prepared_c, None, 3)
    assert len(calls) == 3 and opt_c.step_count == 3
    for (k, va), vc in zip(pol_a.state_dict().items(), pol_c.state_dict().values()):
        assert torch.equal(va, vc), k
    assert dq_c.temp_loss == dq_a.temp_loss
    a_c = dq_c._arena.view("a", prepared_c[2]["N"], torch.float64)
    assert torch.equal(a_c, spy["aa"]) and torch.equal(dq_c._arena.view("y", prepared_c[2]["N"], torch.float64), spy["ya"])
    assert not prepared_c[0]["csr"]
    # ... and from a pool that cached every graph's normalisation / CSRs / AX when its export was stored
    # (drlgx_replay_cache_csr, drlgx_gcn_collate_csr, drlgx_gcn_forward_prebuilt): the same rows in the same order, bit-equal
    pol_d = copy.deepcopy(tgt)
    dq_d = DeepQ("d/", "GCN", data_root=str(tmp_path))
    dq_d.BATCH = B
    dq_d.buffer.extend([(PoolRef(pool_cached, t[0].slot, t[0].env), t[1], t[2], PoolRef(pool_cached, t[3].slot, t[3].env), t[4], t[5]) for t in pooled])
    opt_d = FusedAdam(pol_d.parameters(), lr=1e-3, grad_clamp=dq_d.max_grad_norm)
    it = iter(order)
    prepared_d, _ = dq_d._prepare_updates(3, dev, tgt)
    assert prepared_d[0]["csr"]
    dq_d._train_minibatches(dev, pol_d, tgt, opt_d, prepared_d, None, 3)
    for (k, va), vd in zip(pol_a.state_dict().items(), pol_d.state_dict().values()):
        assert torch.equal(va, vd), k
    assert dq_d.temp_loss == dq_a.temp_loss


def test_batched_graph_build_equals_the_generic_one():
    """drlgx_gcn_forward_batched (both CSRs, degrees and normalised weights of every graph by one workgroup, from the
    batch's graph boundaries) gives the generic build's results bit for bit - forward and all parameter gradients - on
    a batch with explicit self loops, an edge-free graph and one graph of ~10 000 edges (128 KB of sort keys in LDS);
    a bound beyond the kernel's 16 384 edges per graph takes the generic build."""
    from drl_graph_exploration_amd.networks import gcn_trunk
    dev = torch.device("cuda", 0)
    parts = [random_batch(5, 41, dev), random_batch(1, 42, dev, nmin=900, nmax=901), random_batch(3, 43, dev)]
    g = torch.Generator().manual_seed(9)
    n_big = parts[1][0].shape[0]
    extra = torch.randint(0, n_big, (2, 4000), generator=g).to(dev)  # ~10 000 edges in the big graph
    extra = extra[:, extra[0] != extra[1]]
    parts[1] = (parts[1][0], torch.cat([parts[1][1], extra, extra.flip(0)], 1),
                torch.cat([parts[1][2], torch.rand(2 * extra.shape[1], generator=g).to(dev) + 0.1]), parts[1][3])
    xs, eis, eas, node_off, edge_off = [], [], [], [0], [0]
    for x, ei, ea, bt in parts:
        for k in range(int(bt.max()) + 1):
            nodes = torch.nonzero(bt == k).view(-1)
            lo, hi = int(nodes[0]), int(nodes[-1]) + 1
            sel = (ei[0] >= lo) & (ei[0] < hi)
            e, w = ei[:, sel] - lo + node_off[-1], ea[sel]
            if len(xs) == 2:  # explicit self loops in the third graph
                loops = torch.tensor([0, 3], device=dev) + node_off[-1]
                e, w = torch.cat([e, torch.stack([loops, loops])], 1), torch.cat([w, torch.tensor([0.7, 3.1], device=dev)])
            if len(xs) == 4:  # a graph without edges
                e, w = e[:, :0], w[:0]
            xs.append(x[lo:hi]); eis.append(e); eas.append(w)
            node_off.append(node_off[-1] + hi - lo); edge_off.append(edge_off[-1] + e.shape[1])
    x, ei, ea = torch.cat(xs), torch.cat(eis, 1).contiguous(), torch.cat(eas)
    assert max(b - a for a, b in zip(edge_off[:-1], edge_off[1:])) > 8192
    segs = (len(xs), torch.tensor(node_off, dtype=torch.int32, device=dev), torch.tensor(edge_off, dtype=torch.int32, device=dev),
            max(b - a for a, b in zip(edge_off[:-1], edge_off[1:])))
    mask = (torch.rand(x.shape[0], 1000, device=dev) >= 0.5).float() * 2.0
    outs = []
    for s_ in (None, segs, segs[:3] + (20000,)):
        P = make_params(dev, 1)
        out = gcn_trunk(x, ei, ea, P["conv1.weight"], P["conv1.bias"], P["conv2.weight"], P["conv2.bias"], P["fully_con1.weight"],
                        P["fully_con1.bias"], mask, s_)
        (out * torch.linspace(-1, 1, out.numel(), device=dev).view_as(out)).sum().backward()
        outs.append((out.detach(), {k: v.grad.clone() for k, v in P.items()}))
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0])
        for k in outs[0][1]:
            assert torch.equal(outs[0][1][k], o[1][k]), k
    ref = gcn_ref.gcn_forward({k: v.detach() for k, v in make_params(dev, 1).items()}, x, ei, ea, mask)
    assert rel_err(outs[1][0], ref) < 2e-4


def test_hip_heads_and_reward_normalisation_equal_the_tensor_op_forms(monkeypatch):
    """The actor-critic heads as wavefront segment reductions (drlgx_segment_softmax, drlgx_mean_pool, with their
    backward kernels) against the tensor-op forms of the same modules (taken when a batch carries no graph boundaries):
    outputs and all parameter gradients; drlgx_normalise_rewards against the np.interp mirror."""
    import drl_graph_exploration_amd.networks as NW
    from drl_graph_exploration_amd.networks import GraphData, PolicyGCN, ValueGCN
    from drl_graph_exploration_amd.vecenv import normalise_rewards
    dev = torch.device("cuda", 0)
    G = 7
    x, ei, ea, batch = random_batch(G, 55, dev)
    cnt = torch.bincount(batch, minlength=G)
    node_off = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(cnt, 0)]).to(torch.int32)
    ecnt = torch.bincount(batch[ei[0]], minlength=G)
    edge_off = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(ecnt, 0)]).to(torch.int32)
    gen = torch.Generator().manual_seed(2)
    mask = torch.zeros(x.shape[0], dtype=torch.bool)
    for g in range(G):  # the last 1..5 nodes of every graph are its frontier nodes
        mask[int(node_off[g + 1]) - 1 - int(torch.randint(0, 5, (1,), generator=gen)):int(node_off[g + 1])] = True
    mask = mask.to(dev)
    fixed = (torch.rand(x.shape[0], 1000, device=dev) >= 0.5).float() * 2.0
    monkeypatch.setattr(NW, "_dropout_mask", lambda n, hidden, p, device: fixed if p > 0 else None)
    plain = GraphData(x, ei, ea, batch)
    segd = GraphData(x, ei, ea, batch, node_off, edge_off, int(ecnt.max()))
    for cls in (PolicyGCN, ValueGCN):
        torch.manual_seed(1)
        net = cls().to(dev)
        outs = []
        for d in (plain, segd):
            net.zero_grad()
            out = net(d, mask, batch=batch)
            wgt = torch.linspace(0.5, 1.5, out.numel(), device=dev)
            (out * wgt).sum().backward()
            outs.append((out.detach().clone(), [p.grad.clone() for p in net.parameters()]))
        assert outs[0][0].shape == outs[1][0].shape
        assert rel_err(outs[1][0], outs[0][0]) < 1e-5, cls.__name__
        for ga, gb in zip(outs[1][1], outs[0][1]):
            # (the softmax is shift-invariant: the gradient of the read-out bias is round-off around zero in both forms)
            assert float((ga - gb).abs().max()) < 1e-4 * float(gb.abs().max()) + 1e-6, cls.__name__
        if cls is PolicyGCN:  # a distribution per graph
            sums = torch.zeros(G, device=dev).index_add_(0, batch[mask], outs[1][0])
            assert float((sums - 1).abs().max()) < 1e-5
    # reward normalisation
    nfr = torch.tensor([3, 1, 5, 2, 8, 1, 4], dtype=torch.int32)
    first = torch.cumsum(nfr, 0) - nfr
    raw = torch.randn(int(nfr.sum()), dtype=torch.float64, generator=gen)
    raw[first[2]] = raw[first[2]:first[2] + 5].max() + 1.0  # env 2: the nearest frontier is the maximum
    raw[first[4]:first[4] + 8] = 0.25                        # env 4: all equal
    cand_env = torch.repeat_interleave(torch.arange(len(nfr)), nfr.long())
    r_host, l_host = normalise_rewards(raw, cand_env, first.long(), len(nfr))
    r_dev, l_dev = normalise_rewards(raw.to(dev), cand_env.to(dev), first.long().to(dev), len(nfr), nfr.to(dev))
    assert torch.equal(l_dev.cpu(), l_host)
    np.testing.assert_allclose(r_dev.cpu().numpy(), r_host.numpy(), rtol=0, atol=4e-16)
    r_dev2, _ = normalise_rewards(raw.to(dev), cand_env.to(dev), first.long().to(dev), len(nfr))  # counts derived from the offsets
    assert torch.equal(r_dev2, r_dev)


def test_explicit_self_loops_keep_their_weight():
    """PyG add_remaining_self_loops: a node with an explicit self loop keeps that weight instead of the fill value 2
    (gcn_ref.gcn_norm does the same); edges pointing outside the graph are ignored instead of read out of bounds."""
    from drl_graph_exploration_amd.networks import gcn_trunk
    dev = torch.device("cuda", 0)
    x, ei, ea, batch = random_batch(3, 77, dev)
    N = x.shape[0]
    loops = torch.tensor([0, 5, N - 1], device=dev)
    ei2 = torch.cat([ei, torch.stack([loops, loops])], dim=1)
    ea2 = torch.cat([ea, torch.tensor([0.7, 3.1, 1.9], device=dev)])
    P = make_params(dev, 1)
    out = gcn_trunk(x, ei2, ea2, P["conv1.weight"], P["conv1.bias"], P["conv2.weight"], P["conv2.bias"], P["fully_con1.weight"],
                    P["fully_con1.bias"], None)
    ref = gcn_ref.gcn_forward({k: v.detach() for k, v in P.items()}, x, ei2, ea2)
    assert rel_err(out, ref) < 2e-4
    plain = gcn_ref.gcn_forward({k: v.detach() for k, v in P.items()}, x, ei, ea)
    assert rel_err(out, plain) > 1e-3  # the self-loop weights do matter
    bad = torch.tensor([[0, N + 5], [N + 7, 1]], device=dev)
    out2 = gcn_trunk(x, torch.cat([ei2, bad], dim=1), torch.cat([ea2, torch.ones(2, device=dev)]), P["conv1.weight"], P["conv1.bias"],
                     P["conv2.weight"], P["conv2.bias"], P["fully_con1.weight"], P["fully_con1.bias"], None)
    assert torch.equal(out2, out)


def test_a2c_update_without_synchronisations_equals_the_masked_select_form(tmp_path):
    """A2C.train with the frontier mask as a HOST array (the trainer's call: masked positions as gathers, losses accumulated on the device,
    no synchronisation per chunk) against the same update with the mask as a device tensor (policy_cost's masked_select, policy.py:452-458):
    same parameters after the step, same logged loss / entropy, over chunked passes."""
    from drl_graph_exploration_amd.networks import PolicyGCN, ValueGCN, GraphData
    from drl_graph_exploration_amd.policy import A2C
    dev = torch.device("cuda", 0)
    items, masks = [], []
    for k in range(10):
        x, ei, ea, _ = random_batch(1, 40 + k, dev)
        items.append(GraphData(x, ei, ea))
        m = np.zeros(x.shape[0], dtype=bool)
        m[-(3 + k % 4):] = True
        masks.append(m)
    m_all = np.concatenate(masks)
    nn_ = np.array([d.num_nodes for d in items])
    off = np.cumsum(nn_) - nn_
    rng = np.random.RandomState(0)
    a_loc = np.array([int(np.nonzero(m)[0][rng.randint(m.sum())]) for m in masks])
    a_all = np.zeros(m_all.size, dtype=np.float32)
    a_all[off + a_loc] = 1.0
    y_all = np.zeros(m_all.size, dtype=np.float32)
    y_all[off + a_loc] = rng.randn(len(items)).astype(np.float32)
    dr = rng.randn(len(items))
    results = []
    for host_mask in (True, False):
        torch.manual_seed(3)
        a2c = A2C("t%d/" % host_mask, data_root=str(tmp_path))
        a2c.nstep, a2c.graphs_per_pass = 5, 4
        actor, critic = PolicyGCN().to(dev), ValueGCN().to(dev)
        opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=1e-3)
        torch.manual_seed(9)  # (the dropout draws of the passes)
        mask = m_all if host_mask else torch.as_tensor(m_all, device=dev)
        a2c.train(list(items), a_all, mask, dr, y_all, dev, actor, critic, opt, n_traj=2)
        results.append((a2c.temp_loss, a2c.entro, [p.detach().clone() for p in list(actor.parameters()) + list(critic.parameters())]))
    (l0, e0, p0), (l1, e1, p1) = results
    assert abs(l0 - l1) <= 1e-6 * max(1.0, abs(l1)) and abs(e0 - e1) <= 1e-6 * max(1.0, abs(e1)), (l0, l1, e0, e1)
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- edges of the trunk's dispatch
def graph_of(n_nodes, seed, dev):
    """One random graph of exactly n_nodes nodes (a single node has no edge), both directions of every edge."""
    g = torch.Generator().manual_seed(seed)
    m = 0 if n_nodes == 1 else int(torch.randint(n_nodes, 3 * n_nodes, (1,), generator=g))
    src, dst = torch.randint(0, n_nodes, (m,), generator=g), torch.randint(0, n_nodes, (m,), generator=g)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    w = torch.rand(src.shape[0], generator=g) * 5.9 + 0.1
    x = torch.randn(n_nodes, 5, generator=g)
    x[:, 4] = torch.randint(-1, 2, (n_nodes,), generator=g).float()
    return x.to(dev), torch.stack([torch.cat([src, dst]), torch.cat([dst, src])]).to(dev), torch.cat([w, w]).to(dev)


def at_4_bytes(t):
    """A copy of t that starts 4 bytes past a 16-byte boundary (a view into a larger allocation)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def check_trunk_against_float64(x, ei, ea, out_dim, with_mask, unaligned=False, seed=0):
    """gcn_forward_raw / gcn_backward_raw against gcn_ref in float64, under the rule of
    test_gcn_forward_backward_matches_torch_reference.  unaligned: x, Wf and the dropout mask are passed as views at a
    4-byte offset (the trunk's unvectorised branches: k_dz2's scalar loop and thin_tn for read-outs of <= 8 outputs, the
    unvectorised k_gemm for the wider read-out, the 64 x 64 fallback of gemm_wide for the masked layer-2 product)."""
    from drl_graph_exploration_amd.networks import gcn_backward_raw, gcn_forward_raw
    dev = x.device
    N = x.shape[0]
    P = make_params(dev, out_dim, seed)
    mask = None
    if with_mask:
        mask = (torch.rand(N, 1000, device=dev, generator=torch.Generator(device=dev).manual_seed(11 + N)) >= 0.5).float() * 2.0
    names = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fully_con1.weight", "fully_con1.bias")
    params = [P[n].detach() for n in names]
    xk, mk = x, mask
    if unaligned:
        xk, params[4] = at_4_bytes(x), at_4_bytes(params[4])
        mk = at_4_bytes(mask) if mask is not None else None
    out, saved = gcn_forward_raw(xk, ei, ea, params, mk)
    wgt = torch.randn(N, out_dim, device=dev, generator=torch.Generator(device=dev).manual_seed(3 + N))
    grads = [torch.full_like(p, float("nan")) for p in params]
    gcn_backward_raw(saved, wgt, grads)
    torch.cuda.synchronize()
    ref_params = {k: v.detach().double().clone().requires_grad_(True) for k, v in P.items()}
    ref = gcn_ref.gcn_forward(ref_params, x.double(), ei, ea.double(), None if mask is None else mask.double())
    assert out.shape == ref.shape == (N, out_dim)
    assert rel_err(out.double(), ref.detach()) < 1e-5
    with torch.no_grad():
        ref32 = gcn_ref.gcn_forward({k: v.detach() for k, v in P.items()}, x, ei, ea, mask)
    assert rel_err(out, ref32) < 2e-4
    (ref * wgt.double()).sum().backward()
    p32 = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    (gcn_ref.gcn_forward(p32, x, ei, ea, mask) * wgt).sum().backward()
    for name, g in zip(names, grads):
        g, r = g.double(), ref_params[name].grad
        assert torch.isfinite(g).all(), name
        e_ours = float((g - r).norm() / r.norm())
        e_torch32 = float((p32[name].grad.double() - r).norm() / r.norm())
        m_ours, m_torch32 = rel_err(g, r), rel_err(p32[name].grad.double(), r)
        assert m_ours < max(2e-3, 3.0 * m_torch32), (name, m_ours, m_torch32)
        assert e_ours < max(1e-4, 3.0 * e_torch32), (name, e_ours, e_torch32)


@pytest.mark.parametrize("n_nodes,out_dim,with_mask", [(150, 1, True), (150, 8, True), (150, 100, True), (1903, 1, True), (1903, 8, False),
                                                       (1903, 100, True)])
def test_trunk_with_unaligned_operands(n_nodes, out_dim, with_mask):
    """The C ABI takes any pointer: x, Wf and the dropout mask 4 bytes off a 16-byte boundary (1 903 nodes: the tall-tile
    batches, whose aligned products take k_gemm_wide)."""
    dev = torch.device("cuda", 0)
    x, ei, ea = batch_of_about(n_nodes, 500 + n_nodes, dev)
    check_trunk_against_float64(x, ei, ea, out_dim, with_mask, unaligned=True, seed=out_dim)


@pytest.mark.parametrize("out_dim", [9, 12, 16, 17])
def test_trunk_read_out_widths(out_dim):
    """Widths just above the one-pass kernels' 8 outputs, and K = out_dim below / at / just above one 16-wide K slice of the
    dZ2 product."""
    dev = torch.device("cuda", 0)
    x, ei, ea = batch_of_about(300, 600 + out_dim, dev)
    check_trunk_against_float64(x, ei, ea, out_dim, True, seed=out_dim)


@pytest.mark.parametrize("n_nodes", [1, 2, 3, 5, 63, 64, 65, 129])
@pytest.mark.parametrize("out_dim", [1, 100])
def test_trunk_tiny_batches(n_nodes, out_dim):
    """A single node without edges, and node counts around the 64-row tiles."""
    dev = torch.device("cuda", 0)
    x, ei, ea = graph_of(n_nodes, 700 + n_nodes, dev)
    assert (ei.shape[1] == 0) == (n_nodes == 1)
    check_trunk_against_float64(x, ei, ea, out_dim, n_nodes % 2 == 1, seed=n_nodes)


_SWITCH_CHILD = """
import sys, torch
sys.path.insert(0, sys.argv[1])
import test_gpu_gcn as T
dev = torch.device("cuda", 0)
for n, out_dim in ((65, 1), (129, 100), (1101, 1), (1903, 100), (3050, 1)):
    x, ei, ea = T.batch_of_about(n, 900 + n, dev)
    T.check_trunk_against_float64(x, ei, ea, out_dim, True, seed=n)
"""


def test_gemm_development_switches_compute_the_same_trunk():
    """DRLGX_GEMM_DL=0, DRLGX_GEMM_TILE=1, DRLGX_GEMM_WIDE=0 and DRLGX_GEMM_WIDE=6..10 (read once per process) each in a
    fresh process, one after the other: the trunk against float64 at node counts on the 64-row and the tall tiles' edges.
    Stops at the first child that fails, times out or dies by a signal."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for name, value in [("DRLGX_GEMM_DL", "0"), ("DRLGX_GEMM_TILE", "1"), ("DRLGX_GEMM_WIDE", "0")] + \
                       [("DRLGX_GEMM_WIDE", str(v)) for v in range(6, 11)]:
        env = dict(os.environ, **{name: value})
        try:
            r = subprocess.run([sys.executable, "-c", _SWITCH_CHILD, here], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail("%s=%s: the child process timed out" % (name, value))
        assert r.returncode == 0, "%s=%s: exit status %d\n%s" % (name, value, r.returncode, (r.stdout + r.stderr)[-3000:])
