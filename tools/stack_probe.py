#!/usr/bin/env python3
"""What one call for the whole GCN stack (sgx_stack_forward, csrc/stack.hip) saves against one launch per stage.

Two workloads, eval forward of MOL cell 18's model (7 -> 64 ReLU -> 64, mean pool, 64 -> 2 head), fp16:
  mutag    the 188-graph MUTAG batch;
  big      MUTAG's graphs repeated to --graphs graphs (default 1,000,160: 5,320 copies, 17.9 M nodes, 39.6 M edges).
Each is timed chained (ops.layer_forward x 2 + ops.readout_mean_linear, plans as the layer path builds them) and fused
(ops.gcn_stack_forward), eagerly and replayed from a hipGraph, with hipEvents around --reps calls after warm-up (median
of --trials); the outputs of the two are checked bit-equal first.  One JSON line per measurement.

    python tools/stack_probe.py > stack.jsonl
    python tools/stack_probe.py --only big --form fused --reps 5 --trials 1    # one form only, for a counter run
    python tools/stack_probe.py --gat > gat_stack.jsonl
        --gat = the eval forward of sgrace.GAT_POOL_PYNQ (7 -> 64 GAT ReLU -> 64 GAT, mean pool, head; fp16) on the same two
        workloads: "chained" is the model with register layer_count 1 (its layer-by-layer path: per layer X.W and the edge
        softmax aggregate, then the readout), "fused" the same model with layer_count 2 (ops.gat_stack_forward, one launch).
        The two are checked against each other loosely only (the attention path's order is not pinned).
    python tools/stack_probe.py --gat --quant 8 > quant_stack.jsonl
        --quant N = that model with the quantiser on (config.fake_quantization = 1, w_qbits = N, fp32 buffers; without
        --gat its GCN layers): "chained" is the layer-by-layer path (per layer the quantiser passes over W, the attention
        vector and X, X.W, the scores, the aggregate; then the readout), "fused" ops.quant_stack_forward, one launch.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgracex1_amd import graphed, molecule_gcn as M, ops, pyg_lite as G  # noqa: E402

DT = torch.float16


def mutag_batch(copies, dev):
    raw = np.load(os.path.join(ROOT, "tests", "golden", "mutag_raw.npz"))
    b = G.collate(G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"]))
    n, e = b.num_nodes, b.edge_index.shape[1]
    k = torch.arange(copies).repeat_interleave(e)
    ei = b.edge_index.repeat(1, copies) + (k * n).unsqueeze(0)
    batch = b.batch.repeat(copies) + torch.arange(copies).repeat_interleave(n) * b.num_graphs
    return b.x.repeat(copies, 1).to(dev), ei.to(dev), batch.to(dev), b.num_graphs * copies


def setup(copies, dev):
    x, ei, batch, n_graphs = mutag_batch(copies, dev)
    adj = ops.csr_from_edge_index(ei, x.shape[0], dtype=DT)
    fea = M.as_csr(x, DT)
    ptr = ops.graph_ptr_of(batch)
    torch.manual_seed(12345)
    w1, w2 = (torch.randn(64, 7, device=dev) * 0.4).to(DT), (torch.randn(64, 64, device=dev) * 0.15).to(DT)
    hw, hb = torch.randn(2, 64, device=dev), torch.randn(2, device=dev)

    def chained():
        d1 = ops.layer_forward(adj, fea, w1, relu=True)
        d2 = ops.layer_forward(adj, d1, w2, relu=False)
        return ops.readout_mean_linear(d2, ptr, hw, hb)

    def fused():
        return ops.gcn_stack_forward(adj, fea, [w1, w2], [True, False], ptr, hw, hb)

    return dict(chained=chained, fused=fused, n_graphs=n_graphs, nodes=x.shape[0], edges=adj.nnz, adj=adj, ptr=ptr)


def setup_gat(copies, dev, attention=1, quant=0):
    from sgracex1_amd import config, sgrace
    config.acc, config.compute_attention, config.float_type = 1, attention, np.float32 if quant else np.float16
    if quant:
        config.fake_quantization, config.w_qbits = 1, quant
    ip = sgrace.init_SGRACE()
    x, ei, batch, n_graphs = mutag_batch(copies, dev)
    torch.manual_seed(12345)
    model = sgrace.GAT_POOL_PYNQ(7, 64, 2).to(dev).eval()

    def run(layer_count):
        def fn():
            ip.register_map.layer_count = layer_count
            with torch.no_grad():
                return model(x, ei, batch)
        return fn

    run(1)()                                               # builds the cached adjacency the plan below is for
    _ei, _norm, adj = ops.recorded(ei, ("sym_norm2", x.shape[0], 1, torch.float32 if quant else DT))
    return dict(chained=run(1), fused=run(2), n_graphs=n_graphs, nodes=x.shape[0], edges=adj.nnz, adj=adj,
                ptr=ops.graph_ptr_of(batch))


def time_ms(fn, reps, trials):
    out = []
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["mutag", "big"], default=None)
    ap.add_argument("--form", choices=["chained", "fused"], default=None)
    ap.add_argument("--graphs", type=int, default=1_000_160)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--gat", action="store_true")
    ap.add_argument("--quant", type=int, choices=[8, 4, 2, 1], default=0)
    args = ap.parse_args()
    dev = torch.device("cuda")
    work = [("mutag", 1), ("big", max(1, args.graphs // 188))]
    for name, copies in work:
        if args.only and name != args.only:
            continue
        model = args.gat or args.quant
        s = setup_gat(copies, dev, int(args.gat), args.quant) if model else setup(copies, dev)
        plan = ops.BatchPlan.cached(s["adj"], s["ptr"], 64)
        if args.quant and not args.gat:
            assert torch.equal(s["chained"]().view(torch.int32), s["fused"]().view(torch.int32)), "fused != chained"
        elif model:
            assert torch.allclose(s["chained"](), s["fused"](), rtol=1e-2, atol=1e-2), "fused far from chained"
        else:
            assert torch.equal(s["chained"]().view(torch.int32), s["fused"]().view(torch.int32)), "fused != chained"
        reps = args.reps if name == "mutag" else max(1, args.reps // 10)
        for form in ("chained", "fused"):
            if args.form and form != args.form:
                continue
            fn = s[form]
            for _ in range(3):
                fn()
            rec = {"workload": name, "form": form, "graphs": s["n_graphs"], "nodes": s["nodes"], "edges": s["edges"],
                   "plan_groups": plan.groups, "plan_rows": plan.rows, "dtype": "f32" if args.quant else "f16",
                   "model": "GAT_POOL_PYNQ" if model else "GCN"}
            if model:
                rec["attention"] = int(args.gat)
            if args.quant:
                rec["w_qbits"] = args.quant
            rec["eager_ms"] = time_ms(fn, reps, args.trials)
            g = graphed.Graphed(fn)
            rec["graph_ms"] = time_ms(g, reps, args.trials)
            rec["graphs_per_s_eager"] = s["n_graphs"] / (rec["eager_ms"] * 1e-3)
            print(json.dumps(rec), flush=True)
            del g


if __name__ == "__main__":
    main()
