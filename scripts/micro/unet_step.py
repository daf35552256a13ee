"""g-U-Net trunk timings on one GPU (HIP events, warm, median of several repeats): forward, and forward + backward, of a 256-graph
batch at ~60 nodes per graph (depth 3, hidden 1000, ratio 0.5) through drlgx_unet_forward / _backward, beside the HIP GCN trunk
on the same batch in the same session.  The g-U-Net call reads the levels' sizes back once per call, so its times include that
synchronisation.

    python scripts/micro/unet_step.py [--repeats 9] > profiles/unet_step.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

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
    return torch.cat(xs).to(dev), torch.cat(eis, 1).to(dev), torch.cat(eas).to(dev), (n_graphs, no, eo, max(ecounts)), (n_graphs, no, eo, max(sizes))


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
    ap.add_argument("--graphs", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    unet, gcn = NW.GraphUNet(5, 1000, 1000, 3).to(dev), NW.GCN().to(dev)
    up, cp = tuple(p.detach() for p in unet.trunk_parameters()), tuple(p.detach() for p in gcn.trunk_parameters())
    ugrads, cgrads = tuple(torch.empty_like(p) for p in up), tuple(torch.empty_like(p) for p in cp)
    x, ei, ea, gcn_segs, unet_segs = batch_of(args.graphs, 17 + args.graphs, dev)
    N = x.shape[0]
    mask = (torch.rand(N, 1000, device=dev) >= 0.5).float() * 2.0
    d_out = torch.randn(N, 1, device=dev)
    for name, backward in (("forward", False), ("forward_backward", True)):
        def hip_unet():
            out, saved = NW.unet_forward_raw(x, ei, ea, up, 3, 0.5, mask, unet_segs)
            if backward:
                NW.unet_backward_raw(saved, d_out, ugrads)

        def hip_gcn():
            out, saved = NW.gcn_forward_raw(x, ei, ea, cp, mask, gcn_segs)
            if backward:
                NW.gcn_backward_raw(saved, d_out, cgrads)

        row = {"case": name, "graphs": args.graphs, "nodes": N, "edges": int(ei.shape[1])}
        for key, fn in (("hip_unet_ms", hip_unet), ("hip_gcn_ms", hip_gcn)):
            med, lo, hi = timed(fn, args.repeats)
            row[key] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
