"""CPU checks of oracle/train_ref.py, the float64 restatements the trainer-kernel tests compare against: each one
against the primitive it restates (autograd, torch.optim.Adam, np.nanargmax / np.interp, the DQN target loop)."""
import numpy as np
import pytest
import torch

from oracle import dqn_ref, train_ref


def _batch(sizes, rng, p_sel=0.4):
    node_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(node_off[-1])
    return node_off, rng.uniform(-3, 3, n), rng.random(n) < p_sel


def test_segment_softmax_and_backward_equal_autograd():
    rng = np.random.default_rng(0)
    node_off, q, mask = _batch([0, 1, 5, 64, 65, 130, 7], rng)
    mask[1:6] = False  # a graph without a selected node (nodes 1..5)
    batch = np.repeat(np.arange(len(node_off) - 1), np.diff(node_off))
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    sel = torch.tensor(mask)
    b = torch.tensor(batch)[sel]
    qs = qt[sel]
    mx = torch.full((len(node_off) - 1,), -float("inf"), dtype=torch.float64).scatter_reduce(0, b, qs, reduce="amax")
    e = (qs - mx[b]).exp()
    s = torch.zeros(len(node_off) - 1, dtype=torch.float64).index_add(0, b, e)
    p = e / (s[b] + 1e-16)
    np.testing.assert_allclose(train_ref.segment_softmax(q, mask, node_off), p.detach().numpy(), rtol=1e-14, atol=0)
    dp = rng.standard_normal(int(mask.sum()))
    p.backward(torch.tensor(dp))
    dq = train_ref.segment_softmax_backward(p.detach().numpy(), dp, mask, node_off)
    np.testing.assert_allclose(dq, qt.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert np.all(dq[~mask] == 0)


def test_segment_softmax_backward_of_a_rebased_slice():
    """node_off not starting at 0 (a chunk of a larger batch): the output offset is the selected count in front."""
    rng = np.random.default_rng(1)
    node_off, q, mask = _batch([30, 40, 50], rng)
    p = train_ref.segment_softmax(q, mask, node_off)
    dp = rng.standard_normal(p.size)
    full = train_ref.segment_softmax_backward(p, dp, mask, node_off)
    tail = train_ref.segment_softmax_backward(p, dp, mask, node_off[1:])
    assert np.array_equal(tail[30:], full[30:]) and np.all(tail[:30] == 0)


def test_mean_pool_equals_the_index_add_form():
    rng = np.random.default_rng(2)
    node_off = np.array([0, 0, 1, 8, 8, 25])
    h = rng.standard_normal((25, 3))
    batch = torch.tensor(np.repeat(np.arange(5), np.diff(node_off)))
    ht = torch.tensor(h, requires_grad=True)
    s = torch.zeros(5, 3, dtype=torch.float64).index_add(0, batch, ht)
    cnt = torch.zeros(5, dtype=torch.float64).index_add(0, batch, torch.ones(25, dtype=torch.float64))
    v = (s / cnt.clamp(min=1).unsqueeze(1)).mean(dim=1)
    np.testing.assert_allclose(train_ref.mean_pool(h, node_off), v.detach().numpy(), rtol=1e-14, atol=0)
    dv = rng.standard_normal(5)
    v.backward(torch.tensor(dv))
    np.testing.assert_allclose(train_ref.mean_pool_backward(dv, node_off, 3), ht.grad.numpy(), rtol=1e-14, atol=0)


def _rewards_all_goals(frontier_rewards, key_size):
    """What rewards_all_goals does with one env's rewards: NaN for the pose keys, the frontiers' values behind them; the
    nearest frontier is the first; the arg-max decides the target interval of np.interp; NaN entries become 0."""
    rewards = np.array([np.nan] * key_size + list(frontier_rewards))
    nearest_is_best = np.nanargmax(rewards) == key_size
    span = (np.nanmin(rewards), np.nanmax(rewards))
    out = np.interp(rewards, span, (-1.0, 0.0) if nearest_is_best else (-1.0, 1.0))
    out[np.isnan(out)] = 0
    return out[key_size:], not nearest_is_best


def test_normalise_rewards_equals_the_per_env_nanargmax_interp():
    rng = np.random.default_rng(3)
    envs = [rng.uniform(-20, 5, 1), rng.uniform(-20, 5, 70), np.array([3.0, 1.0, 3.0]), np.array([1.0, 3.0, 3.0]),
            np.full(5, -2.5), np.array([0.0, -0.0]), np.array([-0.0, 0.0]), np.array([]), rng.uniform(-1, 1, 200)]
    envs[1][0] = envs[1].max() + 1.0  # nearest frontier is the arg-max
    raw = np.concatenate(envs)
    nf = np.array([len(e) for e in envs])
    first = np.concatenate([[0], np.cumsum(nf)[:-1]])
    out, loop = train_ref.normalise_rewards(raw, first, nf)
    for e, vals in enumerate(envs):
        if not len(vals):
            assert not loop[e]
            continue
        for key_size in (0, 4):
            want, want_loop = _rewards_all_goals(vals, key_size)
            assert loop[e] == want_loop, e
            assert np.array_equal(out[first[e]:first[e] + nf[e]], want), e
    assert [bool(v) for v in loop[:7]] == [False, False, False, True, False, False, False]


def test_dqn_targets_and_cost_equal_the_reference_loop():
    """The [lo, hi) window form against dqn_ref's restatement of the reference loop (start_p over the current-state node
    counts, the last action_space entries of the next-state read-out)."""
    rng = np.random.default_rng(4)
    B = 9
    node_space = rng.integers(3, 12, B)
    action_space = np.minimum(rng.integers(1, 12, B), node_space)
    acts = []
    for i in range(B):
        a = np.zeros(node_space[i])
        a[rng.integers(0, node_space[i])] = 1
        acts.append(a)
    terminals = rng.random(B) < 0.3
    rewards = rng.standard_normal(B)
    readout = rng.standard_normal((int(node_space.sum()), 1)).astype(np.float32)
    a_ref, y_ref = dqn_ref.reference_targets(acts, rewards, terminals, action_space, readout, 0.99)
    start = np.concatenate([[0], np.cumsum(node_space)[:-1]])
    lo, hi = start + node_space - action_space, start + node_space
    pos = start + np.array([int(np.argmax(a)) for a in acts])
    a, y = train_ref.dqn_targets(readout.reshape(-1), lo, hi, pos, terminals, rewards, 0.99, int(node_space.sum()))
    assert np.array_equal(a, a_ref) and np.array_equal(y, y_ref)
    pred = rng.standard_normal(a.size).astype(np.float32)
    loss, d = train_ref.dqn_loss_grad(pred, a, y, B)
    assert abs(loss - dqn_ref.reference_cost(pred, y, a, B)) <= 1e-14 * loss
    pt = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    ((pt * torch.tensor(a) - torch.tensor(y)) ** 2).sum().div(B).backward()
    np.testing.assert_allclose(d, pt.grad.numpy(), rtol=1e-15, atol=0)


@pytest.mark.parametrize("clamp,scale", [(0.0, 1.0), (0.5, 1.0), (0.5, 0.5)])
def test_adam_step_equals_torch_adam_in_float64(clamp, scale):
    rng = np.random.default_rng(5)
    shapes = [(1,), (3,), (1025,), (40, 30)]
    ps = [torch.tensor(rng.standard_normal(s), requires_grad=True) for s in shapes]
    opt = torch.optim.Adam(ps, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    state = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in ps]
    for step in range(1, 6):
        grads = [rng.standard_normal(s) * 1.5 for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g).mul_(scale)
            if clamp > 0:
                p.grad.clamp_(-clamp, clamp)
        opt.step()
        state = [train_ref.adam_step(p, g, m, v, 3e-3, 0.9, 0.999, 1e-8, step, clamp, scale) for (p, m, v), g in zip(state, grads)]
        for p, (pr, mr, vr) in zip(ps, state):
            st = opt.state[p]
            np.testing.assert_allclose(pr, p.detach().numpy(), rtol=1e-14, atol=1e-16)
            np.testing.assert_allclose(mr, st["exp_avg"].numpy(), rtol=1e-13, atol=1e-16)
            np.testing.assert_allclose(vr, st["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-18)


def test_replay_collate_equals_concatenated_graphs():
    rng = np.random.default_rng(6)
    # three graphs stored out of order in the pool, the middle one without edges, ids relative to loc = 10 / 0 / 7
    pool_x = rng.standard_normal((20, 5)).astype(np.float32)
    pool_ei = np.zeros((2, 12), dtype=np.int64)
    pool_ei[:, 0:4] = [[10, 11, 12, 10], [11, 10, 10, 12]]  # graph at rows 12..14, loc 10
    pool_ei[:, 6:9] = [[7, 8, 9], [8, 9, 7]]  # graph at rows 2..4, loc 7
    pool_ea = rng.random(12).astype(np.float32)
    pool_q = rng.standard_normal(20).astype(np.float32)
    desc = np.array([[12, 0, 2], [3, 2, 3], [0, 4, 6], [4, 0, 3], [10, 0, 7]])
    out = train_ref.replay_collate(desc, pool_x, pool_ei, pool_ea, pool_q)
    assert out["node_off"].tolist() == [0, 3, 5, 8] and out["edge_off"].tolist() == [0, 4, 4, 7]
    assert np.array_equal(out["x"], np.concatenate([pool_x[12:15], pool_x[0:2], pool_x[2:5]]))
    assert out["edge_index"].tolist() == [[0, 1, 2, 0, 5, 6, 7], [1, 0, 0, 2, 6, 7, 5]]
    assert np.array_equal(out["edge_attr"], np.concatenate([pool_ea[0:4], pool_ea[6:9]]))
    assert out["batch"].tolist() == [0, 0, 0, 1, 1, 2, 2, 2]
    assert np.array_equal(out["q"], np.concatenate([pool_q[12:15], pool_q[0:2], pool_q[2:5]]))
