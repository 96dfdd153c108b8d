#!/usr/bin/env python3
"""The layers on the entry-split schedule beside the routes a user has without it; one JSON line per run.

    python3 tools/layer_flat_probe.py [--legs a,b,c] [--rounds 3] > profiles/r30_layer_flat.jsonl

Every figure comes from a process of its own (this script starts itself with --child), the routes of a leg alternating
over --rounds rounds, so that a leg's lines show the run-to-run spread beside the gap between routes.

  a  the node example's training step at batch 128 and fan-outs [100, 10], GCN and attention, fp32:
       flat-replayed   NeighborLoader(pad=True, schedule="flat", transposed=True) through NodeTrainer.capture_loader, ms
                       per step of a replayed epoch
       eager-prepared  the prepared loader (no pad: it cannot pad this fan-out without the keyword) through
                       NodeTrainer.step.  This route does not use the feature and runs on the parent commit as well: run
                       the script there with --legs a --routes eager-prepared for the parent's column.
  b  one lean GAT training step (forward + backward of one 256-wide GATConv_SGRACE, no tail) on the arxiv-sized R-MAT
     graph: flat-recorded (flat-marked adjacency, the step recorded and replayed) and planned (eager, the plans built
     outside the timing).  The unplanned route is not a leg: no switch makes the autograd Function run a matrix of 2^20
     entries and more without a plan, so it is reported as not measured.
  c  the same on the arxiv-sized uniform graph, where the entry-split forms are known to lose
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

ROUTES = {"a": ("flat-replayed", "eager-prepared"), "b": ("flat-recorded", "planned"), "c": ("flat-recorded", "planned")}


def _wall_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _configure(attention):
    import numpy as np
    from sgracex1_amd import config, sgrace
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, int(attention)
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 0, "cuda"
    sgrace.init_SGRACE()


def leg_a(route, attention):
    import torch
    from sgrace_node_classification import planted_partition
    from sgracex1_amd import pyg_lite, sgrace
    from sgracex1_amd.train import NodeTrainer
    _configure(attention)
    torch.manual_seed(1)
    n = 3000
    x, edge_index, y = planted_partition(n, 5, 200, 0.2, 0.02, 1, torch.device("cuda"))
    train = torch.zeros(n, dtype=torch.bool, device="cuda")
    train[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:1280].cuda()] = True      # ten full batches
    data = pyg_lite.NodeData(x, edge_index, y, train_mask=train)
    model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).cuda().train()
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=1)
    kw = dict(batch_size=128, input_nodes=train, shuffle=True, seed=1, prepare="sym_norm2", fill=1, transposed=True)
    if route == "flat-replayed":
        loader = pyg_lite.NeighborLoader(data, [100, 10], pad=True, schedule="flat", **kw)
        epoch = trainer.capture_loader(loader)
    else:
        loader = pyg_lite.NeighborLoader(data, [100, 10], **kw)

        def epoch():
            return [trainer.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size) for b in loader]
    epoch()
    ms = [_wall_ms(epoch, 1) / len(loader) for _ in range(5)]
    return {"ms_per_step": [round(v, 4) for v in sorted(ms)], "steps_per_epoch": len(loader)}


def leg_bc(leg, route):
    import torch
    from sgracex1_amd import graphs, ops, sgrace
    _configure(True)
    dev = torch.device("cuda")
    make = graphs.rmat_graph_n if leg == "b" else graphs.uniform_graph
    A = make(169_343, 2_330_000, seed=5, device=dev, dtype=torch.float32)
    n = A.n_rows
    # no dead-row read-back in any route: the fact is given (rows without an entry take the mean row)
    dead = (A.rowptr[1:] == A.rowptr[:-1])
    A.with_facts(dead_row_mask=dead, has_dead_rows=bool(dead.any()))
    if route == "flat-recorded":
        A.with_facts(flat=True)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    layer = sgrace.GATConv_SGRACE(256, 256).to(dev)
    x = (torch.rand((n, 256), generator=g, device=dev) - 0.5).requires_grad_(True)
    G = torch.randn((n, 256), generator=g, device=dev)

    def step():
        layer.weight.grad = layer.attention.grad = x.grad = None
        layer(1, 1, 0, x, None, A.val, A).backward(G)

    step()
    step()
    run = step
    if route == "flat-recorded":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
        run = graph.replay
    ms = sorted(_wall_ms(run, 5) for _ in range(4))
    deg = A.rowptr[1:] - A.rowptr[:-1]
    return {"ms_per_step": [round(v, 4) for v in ms], "rows": n, "entries": A.nnz, "longest_row": int(deg.max()),
            "plans_on_adjacency": A._plan is not None or getattr(A, "_gat_plan", None) is not None}


def child(leg, route, attention):
    rec = {"leg": leg, "route": route, "attention": bool(attention)}
    rec.update(leg_a(route, attention) if leg == "a" else leg_bc(leg, route))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--routes", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs=3, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]))
    for leg in a.legs.split(","):
        routes = a.routes.split(",") if a.routes else ROUTES[leg]
        for attention in ((0, 1) if leg == "a" else (1,)):
            for rnd in range(a.rounds):
                for route in routes:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, route, str(attention)],
                                       capture_output=True, text=True, timeout=600)
                    line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else json.dumps(
                        {"leg": leg, "route": route, "attention": bool(attention), "failed": r.returncode,
                         "stderr": r.stderr.strip().splitlines()[-1:] })
                    print(json.dumps(dict(json.loads(line), round=rnd)), flush=True)
                    if r.returncode != 0:
                        return 1                    # nothing more is started on the device after a failed run
    return 0


if __name__ == "__main__":
    sys.exit(main())
