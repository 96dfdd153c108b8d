#!/usr/bin/env python3
"""What a WHOLE small-graph training step costs -- forward, loss, backward and the optimiser -- with the tail in torch
(F.dropout, Linear, CrossEntropyLoss, autograd, torch.optim.Adam) and with train.StackTrainer (sgx_head_loss,
sgx_adam_step), eager and replayed from one capture.  One process per line, one JSON line per process:

    python tools/train_step_probe.py --model gcn --leg loop      [--tree DIR]     # crit(model(...)), backward, Adam.step()
    python tools/train_step_probe.py --model gcn --leg trainer                    # trainer.step, eager
    python tools/train_step_probe.py --model gcn --leg replay                     # trainer.capture, replayed
    python tools/train_step_probe.py --model gat --leg loop --batch-size 64       # shuffled batches through GraphLoader

--model gcn = GCN_PYNQ in fp16, --model gat = GAT_POOL_PYNQ in fp32, both with train_stack on MUTAG (188 graphs; one
fixed batch, or shuffled batches of --batch-size).  --tree DIR imports the package from another checkout that has been
built (the parent commit's tree, for the leg that shows the run-to-run spread against this tree's `loop`).  Timing as
tools/stack_train_probe.py: hipEvents around --reps steps after a warm-up, median of --trials; the shuffled legs time
whole epochs on the host clock closed by a device synchronisation.  Run every leg twice: the spread belongs on the page.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["gcn", "gat"], default="gcn")
    ap.add_argument("--leg", choices=["loop", "trainer", "replay"], default="loop")
    ap.add_argument("--batch-size", type=int, default=0)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if args.leg == "replay" and args.batch_size:
        ap.error("a replay is the step of one fixed batch")
    root = os.path.abspath(args.tree)
    sys.path.insert(0, root)
    from sgracex1_amd import molecule_gcn as M, pyg_lite as G, pynq_shim

    dev = torch.device("cuda")
    raw = np.load(os.path.join(HERE, "tests", "golden", "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    if args.model == "gat":
        from sgracex1_amd import config, sgrace
        config.acc, config.compute_attention, config.float_type = 1, 1, np.float32
        sgrace.init_SGRACE().register_map.layer_count = 2
        torch.manual_seed(12345)
        net = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(dev).train()
        forward = lambda b: net(b.x, b.edge_index, b.batch)
    else:
        ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
        ip.register_map.layer_count = 2
        net = M.GCN_PYNQ(64, 7, 2, ip, train_stack=True).to(dev).train()
        forward = lambda b: net(1, b.x, b.edge_index, b.batch)
    if args.batch_size:
        gen = torch.Generator().manual_seed(12345)
        kw = dict(dtypes=(torch.float32,), prepare="sym_norm2") if args.model == "gat" else {}
        loader = G.GraphLoader(graphs, batch_size=args.batch_size, shuffle=True, generator=gen, device=dev, **kw)
    else:
        loader = [G.collate(graphs).to(dev)]

    if args.leg == "loop":
        opt = torch.optim.Adam(net.parameters(), lr=0.01)
        crit = torch.nn.CrossEntropyLoss()

        def step(b):
            opt.zero_grad()
            loss = crit(forward(b), b.y)
            loss.backward()
            opt.step()
            return loss
    else:
        from sgracex1_amd.train import StackTrainer
        trainer = StackTrainer(net, lr=0.01)
        step = lambda b: trainer.step(b.x, b.edge_index, b.batch, b.y)

    rec = {"model": args.model, "dtype": "f32" if args.model == "gat" else "f16", "leg": args.leg, "batch_size": args.batch_size,
           "tree": "this" if root == HERE else os.path.basename(root), "tag": args.tag}
    if args.batch_size:
        def epoch():
            n = 0
            for b in loader:
                step(b)
                n += 1
            return n
        for _ in range(3):
            epoch()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.trials):
            t0 = time.perf_counter()
            n = sum(epoch() for _ in range(max(1, args.reps // 3)))
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / n * 1e3)
        rec["step_ms"], rec["step_ms_trials"] = float(np.median(out)), [round(v, 4) for v in out]
    else:
        b = loader[0]
        fn = lambda: step(b)
        if args.leg == "replay":
            fn = trainer.capture(b.x, b.edge_index, b.batch, b.y)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.trials):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / args.reps)
        rec["step_ms"], rec["step_ms_trials"] = float(np.median(out)), [round(v, 4) for v in out]
    if args.leg != "loop":
        rec["fused_steps"] = trainer.fused_steps
    rec["graphs"] = len(graphs)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
