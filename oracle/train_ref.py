"""Float64 restatements of the trainer-side kernels (csrc/k_train.hip) - TEST INFRASTRUCTURE ONLY.

Each function is the plain numpy / torch form of one operation, written from the behaviour the kernels' comments cite:
  segment_softmax / _backward   torch_geometric.utils.softmax over each graph's selected nodes (PolicyGCN head)
  mean_pool / _backward         global_mean_pool(h, batch).mean(dim=1) (ValueGCN head)
  normalise_rewards             ExplorationEnv.rewards_all_goals' np.nanargmax + np.interp (exploration_env.py:151-161)
  dqn_targets                   the TD-target loop of policy.py:154-175 in the [lo, hi) window form the kernel takes
  dqn_loss_grad                 DeepQ.cost (policy.py:234-239) and d(cost)/d(pred)
  adam_step                     grad * scale, clamp_(-c, c), then torch's single-tensor Adam
  replay_collate                torch_geometric Batch.from_data_list over graphs held in a pool
Everything is evaluated in float64 from the float32 inputs the kernels see; the kernels' tests compare against these.
"""
import math

import numpy as np


def _segments(node_off):
    node_off = np.asarray(node_off, dtype=np.int64)
    return [(int(node_off[g]), int(node_off[g + 1])) for g in range(len(node_off) - 1)]


def segment_softmax(q, mask, node_off):
    """p over the selected nodes of all graphs, in node order: exp(q - max) / (sum exp(q - max) + 1e-16) per graph."""
    q = np.asarray(q, dtype=np.float64)
    mask = np.asarray(mask).astype(bool)
    out = []
    for n0, n1 in _segments(node_off):
        v = q[n0:n1][mask[n0:n1]]
        if v.size:
            e = np.exp(v - v.max())
            out.append(e / (e.sum() + 1e-16))
    return np.concatenate(out) if out else np.zeros(0)


def segment_softmax_backward(p, dp, mask, node_off):
    """dq over all nodes: p_j (dp_j - sum_i p_i dp_i) on the selected nodes of each graph, 0 elsewhere."""
    p = np.asarray(p, dtype=np.float64)
    dp = np.asarray(dp, dtype=np.float64)
    mask = np.asarray(mask).astype(bool)
    dq = np.zeros(mask.shape[0])
    k = int(mask[:int(np.asarray(node_off)[0])].sum())
    for n0, n1 in _segments(node_off):
        sel = np.nonzero(mask[n0:n1])[0] + n0
        pj, dpj = p[k:k + sel.size], dp[k:k + sel.size]
        dq[sel] = pj * (dpj - math.fsum(pj * dpj))
        k += sel.size
    return dq


def mean_pool(h, node_off):
    """v[g] = mean over the columns of the mean over graph g's rows; an empty graph gives 0."""
    h = np.asarray(h, dtype=np.float64)
    v = np.zeros(len(node_off) - 1)
    for g, (n0, n1) in enumerate(_segments(node_off)):
        if n1 > n0:
            v[g] = h[n0:n1].mean(axis=0).mean()
    return v


def mean_pool_backward(dv, node_off, n_cols):
    """dh[n][c] = dv[g] / (n_g C) for the rows n of graph g."""
    dv = np.asarray(dv, dtype=np.float64)
    no = np.asarray(node_off, dtype=np.int64)
    dh = np.zeros((int(no[-1]), n_cols))
    for g, (n0, n1) in enumerate(_segments(no)):
        if n1 > n0:
            dh[n0:n1] = dv[g] / ((n1 - n0) * n_cols)
    return dh


def normalise_rewards(raw, first, n_frontier):
    """One env at a time, as rewards_all_goals does it: the env's frontier rewards (the first is the vehicle's nearest)
    behind NaN entries for the pose keys, np.nanargmax, then np.interp onto [-1, 0] (the nearest frontier is the arg-max:
    loop_clo False) or [-1, 1] (loop_clo True).  Returns (out over raw's indices - 0 where no env writes -, loop_clo)."""
    raw = np.asarray(raw, dtype=np.float64)
    out = np.zeros_like(raw)
    loop = np.zeros(len(first), dtype=bool)
    for e, (f0, nf) in enumerate(zip(first, n_frontier)):
        f0, nf = int(f0), int(nf)
        if nf <= 0:
            continue
        key_size = 3  # (any number of NaN pose entries in front: they change neither the arg-max rule nor the interpolation)
        rewards = [np.nan] * key_size + list(raw[f0:f0 + nf])
        act_max = np.nanargmax(rewards)
        top = 0.0 if act_max == key_size else 1.0
        loop[e] = act_max != key_size
        r = np.interp(rewards, (np.nanmin(rewards), np.nanmax(rewards)), (-1.0, top))
        out[f0:f0 + nf] = r[key_size:]
    return out, loop


def dqn_targets(q1, lo, hi, pos, terminal, r, gamma, n_total):
    """a_batch[pos_i] = 1, y_batch[pos_i] = r_i (terminal) or r_i + gamma * max(q1[lo_i:hi_i]) (the float32 maximum,
    promoted), both zero elsewhere."""
    q1 = np.asarray(q1, dtype=np.float32)
    a = np.zeros(n_total)
    y = np.zeros(n_total)
    for i in range(len(lo)):
        t = float(r[i])
        if not terminal[i]:
            t = float(r[i]) + gamma * float(np.max(q1[int(lo[i]):int(hi[i])]))
        a[int(pos[i])] = 1.0
        y[int(pos[i])] = t
    return a, y


def dqn_loss_grad(pred, action, y, batch):
    """(sum (pred a - y)^2 / batch with an exactly rounded sum, d_pred = 2 (pred a - y) a / batch in float64)."""
    e = np.asarray(pred, dtype=np.float64) * np.asarray(action, dtype=np.float64) - np.asarray(y, dtype=np.float64)
    return math.fsum(e * e) / batch, 2.0 * e * np.asarray(action, dtype=np.float64) / batch


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, clamp=0.0, scale=1.0):
    """One step of torch.optim.Adam (single-tensor form, no weight decay / amsgrad) on the gradient g * scale clamped to
    [-clamp, clamp] (clamp <= 0: none).  float64 arrays in, new (p, m, v) out."""
    g = np.asarray(g, dtype=np.float64) * scale
    if clamp > 0:
        g = np.clip(g, -clamp, clamp)
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    step_size = lr / (1.0 - beta1 ** step)
    denom = np.sqrt(v) / math.sqrt(1.0 - beta2 ** step) + eps
    return p - step_size * m / denom, m, v


def replay_collate(desc, pool_x, pool_ei, pool_ea, pool_q=None):
    """desc int64 [5][G] = node_start, node_cnt, edge_start, edge_cnt, loc.  Returns dict of x, edge_index [2][E] (node
    ids - loc + the graph's offset in the batch), edge_attr, batch, node_off, edge_off [G + 1] and q (pool_q gathered)."""
    desc = np.asarray(desc, dtype=np.int64)
    xs, eis, eas, bs, qs = [], [], [], [], []
    node_off, edge_off = [0], [0]
    for g in range(desc.shape[1]):
        n0, nn, e0, ne, loc = (int(t) for t in desc[:, g])
        xs.append(pool_x[n0:n0 + nn])
        eis.append(pool_ei[:, e0:e0 + ne] - loc + node_off[-1])
        eas.append(pool_ea[e0:e0 + ne])
        bs.append(np.full(nn, g, dtype=np.int64))
        if pool_q is not None:
            qs.append(pool_q[n0:n0 + nn])
        node_off.append(node_off[-1] + nn)
        edge_off.append(edge_off[-1] + ne)
    out = dict(x=np.concatenate(xs), edge_index=np.concatenate(eis, axis=1), edge_attr=np.concatenate(eas), batch=np.concatenate(bs),
               node_off=np.array(node_off, dtype=np.int64), edge_off=np.array(edge_off, dtype=np.int64))
    if pool_q is not None:
        out["q"] = np.concatenate(qs)
    return out
