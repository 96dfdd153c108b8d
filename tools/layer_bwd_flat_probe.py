#!/usr/bin/env python3
"""The one-call layer backward on the entry-split schedules beside the routes that existed before it; one JSON
line per run.

    python3 tools/layer_bwd_flat_probe.py [--legs a,b,c] [--rounds 3] > profiles/r31_layer_bwd_flat.jsonl

Every figure comes from a process of its own (this script starts itself with --child) under a time limit, the routes of a
leg alternating over --rounds rounds, so that a leg's lines show the run-to-run spread beside the gap between routes.  The
reference route of every leg is code the parent commit has too (its device code is unchanged), never the code under test.

  a  the attention gradient alone on the arxiv-sized R-MAT and uniform graphs at F = 256: `rows` (sgx_gat_attention_grad,
     the parent's) and `flat` (sgx_gat_attention_grad_flat)
  b  one lean GAT training step (forward + backward of one 256-wide GATConv_SGRACE, no tail) on those graphs:
     `accb1-rows` (the parent's one call), `accb1-flat` (flat-marked adjacency) and `accb0` (the parent's default)
  c  the node example's padded replayed step at batch 128, fan-outs [10, 10] and [100, 10], GCN and attention:
     `accb1-flat` against `accb0-flat`, the parent's replay
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

ROUTES = {"a": ("rows", "flat"), "b": ("accb1-rows", "accb1-flat", "accb0"), "c": ("accb0-flat", "accb1-flat")}
CASES = {"a": ("rmat", "uniform"), "b": ("rmat", "uniform"), "c": ("gcn-10,10", "att-10,10", "gcn-100,10", "att-100,10")}
CHILD_LIMIT = 300          # seconds per process


def _wall_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _configure(attention, accb):
    import numpy as np
    from sgracex1_amd import config, sgrace
    config.acc, config.accb, config.float_type, config.compute_attention = 1, int(accb), np.float32, int(attention)
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 0, "cuda"
    sgrace.init_SGRACE()


def _graph(case):
    import torch
    from sgracex1_amd import graphs
    make = graphs.rmat_graph_n if case == "rmat" else graphs.uniform_graph
    return make(169_343, 2_330_000, seed=5, device=torch.device("cuda"), dtype=torch.float32)


def leg_a(route, case):
    import torch
    from sgracex1_amd import ops
    A = _graph(case)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    sg = torch.randn(A.nnz, generator=g, device="cuda")
    g1 = torch.randn(A.n_rows, generator=g, device="cuda")
    Wh = torch.randn((A.n_cols, 256), generator=g, device="cuda")
    schedule = "flat" if route == "flat" else None
    run = lambda: ops.gat_attention_grad(A, sg, g1, Wh, schedule=schedule)
    run()
    ms = sorted(_wall_ms(run, 20) for _ in range(4))
    deg = A.rowptr[1:] - A.rowptr[:-1]
    return {"ms": [round(v, 4) for v in ms], "rows": A.n_rows, "entries": A.nnz, "longest_row": int(deg.max())}


def leg_b(route, case):
    import torch
    from sgracex1_amd import sgrace
    _configure(True, 0 if route == "accb0" else 1)
    A = _graph(case)
    n = A.n_rows
    dead = (A.rowptr[1:] == A.rowptr[:-1])
    A.with_facts(dead_row_mask=dead, has_dead_rows=bool(dead.any()))
    if route == "accb1-flat":
        A.with_facts(flat=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    layer = sgrace.GATConv_SGRACE(256, 256).to("cuda")
    x = (torch.rand((n, 256), generator=g, device="cuda") - 0.5).requires_grad_(True)
    G = torch.randn((n, 256), generator=g, device="cuda")

    def step():
        layer.weight.grad = layer.attention.grad = x.grad = None
        layer(1, 1, 0, x, None, A.val, A).backward(G)

    step()
    step()
    ms = sorted(_wall_ms(step, 5) for _ in range(4))
    return {"ms_per_step": [round(v, 4) for v in ms], "rows": n, "entries": A.nnz,
            "plans_on_adjacency": A._plan is not None or getattr(A, "_gat_plan", None) is not None}


def leg_c(route, case):
    import torch
    from sgrace_node_classification import planted_partition
    from sgracex1_amd import pyg_lite, sgrace
    from sgracex1_amd.train import NodeTrainer
    kind, fan = case.split("-")
    fanouts = [int(k) for k in fan.split(",")]
    _configure(kind == "att", 1 if route == "accb1-flat" else 0)
    torch.manual_seed(1)
    n = 3000
    x, edge_index, y = planted_partition(n, 5, 200, 0.2, 0.02, 1, torch.device("cuda"))
    train = torch.zeros(n, dtype=torch.bool, device="cuda")
    train[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:1280].cuda()] = True      # ten full batches
    data = pyg_lite.NodeData(x, edge_index, y, train_mask=train)
    model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).cuda().train()
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=1)
    loader = pyg_lite.NeighborLoader(data, fanouts, pad=True, schedule="flat", batch_size=128, input_nodes=train, shuffle=True, seed=1,
                                     prepare="sym_norm2", fill=1, transposed=True)
    epoch = trainer.capture_loader(loader)
    epoch()
    ms = [_wall_ms(epoch, 1) / len(loader) for _ in range(5)]
    return {"ms_per_step": [round(v, 4) for v in sorted(ms)], "steps_per_epoch": len(loader)}


def child(leg, route, case):
    rec = {"leg": leg, "route": route, "case": case}
    rec.update({"a": leg_a, "b": leg_b, "c": leg_c}[leg](route, case))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs=3, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    for leg in a.legs.split(","):
        for case in CASES[leg]:
            for rnd in range(a.rounds):
                for route in ROUTES[leg]:
                    try:
                        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, route, case],
                                           capture_output=True, text=True, timeout=CHILD_LIMIT)
                        rc, out, err = r.returncode, r.stdout, r.stderr
                    except subprocess.TimeoutExpired:
                        rc, out, err = 124, "", "time limit"
                    line = out.strip().splitlines()[-1] if rc == 0 and out.strip() else json.dumps(
                        {"leg": leg, "route": route, "case": case, "failed": rc, "stderr": err.strip().splitlines()[-1:]})
                    print(json.dumps(dict(json.loads(line), round=rnd)), flush=True)
                    if rc != 0:
                        return 1                    # nothing more is started on the device after a failed run
    return 0


if __name__ == "__main__":
    sys.exit(main())
