#!/usr/bin/env python3
"""One GAT training step and the 8-head aggregate forward on the ogbn-arxiv shape (169 K nodes, 2.3 M edges, 128 -> 256;
uniform and R-MAT degrees as tools/gat_probe.py builds them), with the per-edge outputs E / S kept for the backward
(config.gat_edge_outputs = 1, the default) and with the row softmax statistics instead (0, "lean"):

    python3 tools/gat_train_probe.py [--legs default,lean] [--label NAME] [--repeats 30] [--tree DIR]
                                     [--accb 0,1] [--gat 0] [--steps-only]

  --accb       config.accb of the step, a comma list run in that order (0,1,0,1 interleaves the two): 0 = the backward
               composed from stage calls, 1 = the one call (sgx_layer_backward); a tree without the call ignores 1
  --gat 0      the GCN aggregate instead of the edge softmax (the step only); --steps-only: no 8-head aggregates

  step   GATConv_SGRACE(128, 256), one head, dense features: forward + backward of FPYNQ_GAT, fp32 and fp16 storage
  agg8   ops.gat_aggregate at 8 heads x 32 columns, forward alone (there is no multi-head backward): with E / S as a
         training forward asks for them today, without side outputs, and (lean) with the statistics
Each figure: 5 warm-up runs, then --repeats runs timed one by one with device events; median, 10th and 90th percentile
(the spread), and torch.cuda.max_memory_allocated over the timed runs.  One JSON line per (graph, dtype, what, leg).
The default leg uses only calls that exist without the statistics path, so --tree DIR runs it on another checkout of the
package (the parent commit, built) for a baseline from the same process layout.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch


def timed(fn, repeats, warmup=5):
    from sgracex1_amd.hipevents import Event
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    s = torch.cuda.current_stream().cuda_stream
    ts = []
    for _ in range(repeats):
        b, e = Event(), Event()
        b.record(s)
        fn()
        e.record(s)
        ts.append(b.elapsed_ms(e))
    ts = np.sort(np.array(ts))
    pick = lambda q: round(float(ts[min(len(ts) - 1, int(q * len(ts)))]), 4)
    return dict(ms_median=pick(0.5), ms_p10=pick(0.1), ms_p90=pick(0.9), repeats=repeats,
                max_memory_MiB=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="default,lean")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--accb", default="0", help="config.accb of the training step, a comma list: 0 = composed, 1 = one call")
    ap.add_argument("--gat", type=int, default=1, choices=[0, 1], help="0: the GCN aggregate instead (steps only)")
    ap.add_argument("--steps-only", action="store_true", help="the training step alone, not the 8-head aggregates")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from sgracex1_amd import config, graphs, ops, sgrace
    dev = torch.device("cuda")
    M, P = 128, 256
    for gname in ("uniform", "rmat"):
        build = graphs.uniform_graph if gname == "uniform" else graphs.rmat_graph_n
        A32 = build(169_343, 2_330_000, seed=5, device=dev, dtype=torch.float32)
        n = A32.n_rows
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        X = torch.rand((n, M), generator=gen, device=dev).half().float()
        G = torch.randn((n, P), generator=gen, device=dev)
        Wh = torch.rand((n, P), generator=gen, device=dev)
        att8 = (torch.rand(2 * P, generator=gen, device=dev) * 2 - 1) * 0.3
        for dt, npdt in ((torch.float32, np.float32), (torch.float16, np.float16)):
            A = A32.to(dt)
            A.gat_plan, A.plan
            for leg, accb in [(l, int(b)) for l in a.legs.split(",") for b in a.accb.split(",")]:
                flag = {"default": 1, "lean": 0}[leg]
                old = config.snapshot()
                try:
                    config.acc, config.compute_attention, config.device, config.float_type = 1, a.gat, "cuda", npdt
                    config.accb = accb
                    config.fake_quantization, config.w_qbits = 0, 32
                    config.gat_edge_outputs = flag
                    sgrace.init_SGRACE()
                    torch.manual_seed(2)
                    layer = sgrace.GATConv_SGRACE(M, P).to(dev)

                    def step():
                        x = X.detach().requires_grad_(True)
                        layer.zero_grad(set_to_none=True)
                        layer(a.gat, 1, 0, x, None, A.val, A).backward(G)          # (A is of the layer's type: no copy per step)

                    res = timed(step, a.repeats)
                finally:
                    config.restore(old)
                    sgrace.init_SGRACE()
                base = dict(label=a.label, graph=gname, nodes=n, edges=A.nnz, dtype=str(dt).split(".")[1], leg=leg, accb=accb,
                            gat=a.gat)
                print(json.dumps(dict(base, what="step_1x256_fwd_bwd", **res)), flush=True)
                if a.steps_only or not a.gat:
                    continue
                Whd, attd = Wh.to(dt), att8.to(dt)
                D = torch.empty((n, P), dtype=dt, device=dev)
                forms = {"default": (("agg8_with_E_S", dict(want_edge_outputs=True)), ("agg8_no_side_outputs", {})),
                         "lean": (("agg8_with_statistics", dict(want_row_stats=True)),)}[leg]
                for what, kw in forms:
                    res = timed(lambda: ops.gat_aggregate(A, Whd, attd, heads=8, out=D, **kw), a.repeats)
                    print(json.dumps(dict(base, what=what, **res)), flush=True)


if __name__ == "__main__":
    main()
