#!/usr/bin/env python3
"""The quantised layers on the entry-split schedule beside the route a user had without it; one JSON line
per run.

    python3 tools/quant_flat_probe.py [--legs a,b] [--rounds 3] > profiles/r32_quant_flat.jsonl

Every figure comes from a process of its own (this script starts itself with --child) under a time limit, the routes of a
leg alternating over --rounds rounds, so that a leg's lines show the run-to-run spread beside the gap between routes.

  a  the node example's QUANTISED training step (8 bits, hardware_quantize = 1) at batch 128 and fan-outs [100, 10], GCN
     and attention:
       flat-replayed   NeighborLoader(pad=True, schedule="flat", quant=qc, flat_quant=True, transposed=True) through
                       NodeTrainer.capture_loader, ms per step of a replayed epoch
       eager-prepared  NeighborLoader(prepare="sym_norm2", quant=qc) through NodeTrainer.step: the only route at this
                       fan-out before the opt-in (the padded loader refuses rows over 64 entries without schedule="flat",
                       and schedule="flat" refused quant=).  It uses nothing new and runs on the parent commit as well.
  b  the aggregation stage alone on the arxiv-sized R-MAT graph, 256 fp32 columns, deq_o on D:
       fused           sgx_spmm_csr_flat_ep(out_scale = deq_o)
       separate        sgx_spmm_csr_flat followed by a scale pass over D (D.mul_)

After a leg's last run one "summary" line follows: the run medians of both routes, the gap from the new route's worst
median to the reference route's best, and the reference route's own run-to-run spread (its medians' range, and the range of
all its samples).  win_claimed is true only when the gap exceeds that spread of medians AND every sample of the new route
lies below every sample of the reference route; a leg whose runs did not all finish gets "not measured" instead.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

ROUTES = {"a": ("flat-replayed", "eager-prepared"), "b": ("fused", "separate")}
CHILD_LIMIT_S = 300


def _wall_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def leg_a(route, attention):
    import numpy as np
    import torch
    from sgrace_node_classification import planted_partition
    from sgracex1_amd import config, pyg_lite, sgrace
    from sgracex1_amd.train import NodeTrainer
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, int(attention)
    config.fake_quantization = config.hardware_quantize = 1
    config.w_qbits, config.gat_edge_outputs, config.device = 8, 0, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(1)
    n = 3000
    x, edge_index, y = planted_partition(n, 5, 200, 0.2, 0.02, 1, torch.device("cuda"))
    train = torch.zeros(n, dtype=torch.bool, device="cuda")
    train[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:1280].cuda()] = True      # ten full batches
    data = pyg_lite.NodeData(x, edge_index, y, train_mask=train)
    model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).cuda().train()
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=1)
    kw = dict(batch_size=128, input_nodes=train, shuffle=True, seed=1, prepare="sym_norm2", fill=1, transposed=True,
              quant=sgrace.quant_constants)
    if route == "flat-replayed":
        loader = pyg_lite.NeighborLoader(data, [100, 10], pad=True, schedule="flat", flat_quant=True, **kw)
        epoch = trainer.capture_loader(loader)
    else:
        loader = pyg_lite.NeighborLoader(data, [100, 10], **kw)

        def epoch():
            return [trainer.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size) for b in loader]
    epoch()
    ms = [_wall_ms(epoch, 1) / len(loader) for _ in range(5)]
    return {"ms_per_step": [round(v, 4) for v in sorted(ms)], "steps_per_epoch": len(loader), "qbits": 8}


def leg_b(route):
    import numpy as np
    import torch
    from sgracex1_amd import graphs, ops, quant
    dev = torch.device("cuda")
    A = graphs.rmat_graph_n(169_343, 2_330_000, seed=5, device=dev, dtype=torch.float32)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    H = torch.rand((A.n_cols, 256), generator=g, device=dev) - 0.5
    out = torch.empty((A.n_rows, 256), device=dev)
    s = float(np.float32(quant.constants(8).deq_o))
    if route == "fused":
        run = lambda: ops.spmm(A, H, relu=True, out=out, schedule="flat", out_scale=s)
    else:
        run = lambda: ops.spmm(A, H, relu=True, out=out, schedule="flat").mul_(s)
    run()
    run()
    ms = sorted(_wall_ms(run, 20) for _ in range(5))
    deg = A.rowptr[1:] - A.rowptr[:-1]
    return {"ms_per_call": [round(v, 4) for v in ms], "rows": A.n_rows, "entries": A.nnz, "longest_row": int(deg.max()), "columns": 256}


def child(leg, route, attention):
    rec = {"leg": leg, "route": route}
    if leg == "a":
        rec["attention"] = bool(attention)
    rec.update(leg_a(route, attention) if leg == "a" else leg_b(route))
    print(json.dumps(rec), flush=True)


def summary(what, new, old, runs):
    """the leg's summary line from its per-run lines (runs: route -> list of sorted sample lists, ms)"""
    if any(len(runs.get(r, [])) == 0 for r in (new, old)):
        return dict(what, summary="not measured")
    med = {r: [statistics.median(v) for v in runs[r]] for r in (new, old)}
    lo = {r: min(min(v) for v in runs[r]) for r in (new, old)}
    hi = {r: max(max(v) for v in runs[r]) for r in (new, old)}
    gap = min(med[old]) - max(med[new])
    spread = max(med[old]) - min(med[old])
    return dict(what, summary="measured", unit="ms", new_route=new, reference_route=old, new_run_medians=med[new],
                reference_run_medians=med[old], new_range=[lo[new], hi[new]], reference_range=[lo[old], hi[old]],
                gap_worst_new_median_to_best_reference_median=round(gap, 4),
                reference_run_to_run_spread_of_medians=round(spread, 4), reference_sample_range=round(hi[old] - lo[old], 4),
                win_claimed=bool(gap > spread and hi[new] < lo[old]),
                note="the reference route uses nothing this change adds: it is the route the parent commit has for this leg, "
                     "run from this tree, alternating with the new route, each run in a process of its own")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs=3, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]))
    for leg in a.legs.split(","):
        routes = ROUTES[leg]
        key = "ms_per_step" if leg == "a" else "ms_per_call"
        for attention in ((0, 1) if leg == "a" else (0,)):
            runs = {r: [] for r in routes}
            for rnd in range(a.rounds):
                for route in routes:
                    what = {"leg": leg, "route": route, **({"attention": bool(attention)} if leg == "a" else {})}
                    try:
                        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, route, str(attention)],
                                           capture_output=True, text=True, timeout=CHILD_LIMIT_S)
                    except subprocess.TimeoutExpired:
                        print(json.dumps(dict(what, failed="time limit", round=rnd)), flush=True)
                        print(json.dumps(dict(what, route=None, summary="not measured")), flush=True)
                        return 1
                    line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else json.dumps(
                        dict(what, failed=r.returncode, stderr=r.stderr.strip().splitlines()[-1:]))
                    print(json.dumps(dict(json.loads(line), round=rnd)), flush=True)
                    if r.returncode != 0:
                        print(json.dumps(dict(what, route=None, summary="not measured")), flush=True)
                        return 1                    # nothing more is started on the device after a failed run
                    runs[route].append(json.loads(line)[key])
            leg_what = {"leg": leg, **({"attention": bool(attention)} if leg == "a" else {})}
            print(json.dumps(summary(leg_what, routes[0], routes[1], runs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
