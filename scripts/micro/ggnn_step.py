"""GG-NN trunk timings on one GPU (HIP events, warm, median of several repeats):
  * forward of a 256-graph export at ~60 nodes per graph (the decision step of the 256-env loop),
  * forward + backward of a 64-graph batch (one update),
each for the HIP trunk (drlgx_ggnn_forward / _backward), for the float32 plain-torch restatement on the GPU (rocBLAS +
index_add_, tests/ggnn_ref.py; backward through autograd) and for the HIP GCN trunk on the same batch.  Also prints the HBM time of
the panels one GRU gate pass touches (7 read + 5 written per node and feature, float32; the last layer reads the mask too) at 6 TB/s for comparison with a
profiler's per-kernel times.

    python scripts/micro/ggnn_step.py [--repeats 9] > profiles/ggnn_step.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ggnn_ref  # noqa: E402
from drl_graph_exploration_amd import networks as NW  # noqa: E402


def batch_of(n_graphs, seed, dev):
    """Graphs of 50..70 nodes, each undirected edge stored in both directions (as the exploration graphs), ~3 per node."""
    g = torch.Generator().manual_seed(seed)
    xs, eis, eas, sizes, ecounts, off = [], [], [], [], [], 0
    for _ in range(n_graphs):
        n = int(torch.randint(50, 71, (1,), generator=g))
        m = 3 * n
        src = torch.randint(0, n, (m,), generator=g)
        dst = (src + 1 + torch.randint(0, n - 1, (m,), generator=g)) % n
        w = torch.rand(m, generator=g) * 0.9 + 0.1
        eis.append(torch.stack([torch.cat([src, dst]), torch.cat([dst, src])]) + off)
        eas.append(torch.cat([w, w]))
        xs.append(torch.randn(n, 5, generator=g))
        sizes.append(n)
        ecounts.append(2 * m)
        off += n
    no = torch.tensor([0] + sizes).cumsum(0).int().to(dev)
    eo = torch.tensor([0] + ecounts).cumsum(0).int().to(dev)
    return torch.cat(xs).to(dev), torch.cat(eis, 1).to(dev), torch.cat(eas).to(dev), (n_graphs, no, eo, max(ecounts))


def timed(fn, repeats, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ggnn, gcn = NW.GGNN().to(dev), NW.GCN().to(dev)
    ref = ggnn_ref.RefGGNN(1000, 3, 1)
    ref.load_state_dict({k: v.cpu() for k, v in ggnn.state_dict().items()})
    ref.to(dev)
    gp, cp = tuple(p.detach() for p in ggnn.trunk_parameters()), tuple(p.detach() for p in gcn.trunk_parameters())
    ggrads, cgrads = tuple(torch.empty_like(p) for p in gp), tuple(torch.empty_like(p) for p in cp)
    for name, n_graphs, backward in (("forward_256_graphs", 256, False), ("forward_backward_64_graphs", 64, True)):
        x, ei, ea, segs = batch_of(n_graphs, 17 + n_graphs, dev)
        N = x.shape[0]
        mask = (torch.rand(N, 1000, device=dev) >= 0.5).float() * 2.0
        d_out = torch.randn(N, 1, device=dev)

        def hip_ggnn():
            out, saved = NW.ggnn_forward_raw(x, ei, ea, gp, mask, segs)
            if backward:
                NW.ggnn_backward_raw(saved, d_out, ggrads)

        def hip_gcn():
            out, saved = NW.gcn_forward_raw(x, ei, ea, cp, mask, segs)
            if backward:
                NW.gcn_backward_raw(saved, d_out, cgrads)

        def torch_ggnn():
            if backward:
                ref.zero_grad(set_to_none=True)
                (ref(x, ei, ea, mask) * d_out).sum().backward()
            else:
                with torch.no_grad():
                    ref(x, ei, ea, mask)

        row = {"case": name, "graphs": n_graphs, "nodes": N, "edges": int(ei.shape[1])}
        for key, fn in (("hip_ggnn_ms", hip_ggnn), ("torch_fp32_ggnn_ms", torch_ggnn), ("hip_gcn_ms", hip_gcn)):
            med, lo, hi = timed(fn, args.repeats)
            row[key] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        row["gate_pass_hbm_us_at_6TBs"] = round(12 * N * 1000 * 4 / 6e12 * 1e6, 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
