#!/usr/bin/env python3
"""What a WHOLE node-classification step of sgrace.GAT_PYNQ costs -- layers, loss, backward and the optimiser -- with the
tail in torch (F.dropout, Linear, CrossEntropyLoss over out[train], autograd, torch.optim.Adam(weight_decay=5e-4)) and
with train.NodeTrainer (sgx_node_loss, sgx_adam_step), eager and replayed from one capture.  One process per line, one JSON
line per process, printed and appended to --out (profiles/r19_node_train.jsonl):

    python tools/node_train_probe.py --graph example --leg loop [--tree DIR]    # crit(model(x, ei)[train], y[train]) ...
    python tools/node_train_probe.py --graph cora --attention --leg trainer     # trainer.step, eager
    python tools/node_train_probe.py --graph arxiv --leg replay                 # trainer.capture, replayed
    python tools/node_train_probe.py --graph example --leg loop --batch-size 128 --num-neighbors 10,10 [--device-batches]
    python tools/node_train_probe.py --graph arxiv --leg kernel                 # the sgx_node_loss call alone

--graph example = the example's planted-partition graph (n = 3000); cora = a random graph of Cora's size (2708 nodes,
1433 sparse features, 7 classes, 140 training rows, 10556 stored edges); arxiv = one of ogbn-arxiv's (169343 nodes, 128
features, 40 classes, 2.5 M stored edges, 90941 training rows).  --tree DIR imports the package from another built
checkout (the parent commit's tree: the leg that shows the run-to-run spread against this tree's `loop`).  Timing:
hipEvents around --reps steps after a warm-up, median of --trials; mini-batch legs time whole epochs on the host clock
closed by a device synchronisation.  Run every leg twice: the spread belongs on the page.  The kernel leg sets the call
against the bytes it must move: H read for the blocks that hold a selected row, grad_H written for every row."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_graph(n, f_in, classes, edges, n_train, density, seed, dev):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (edges // 2,), generator=g), torch.randint(0, n, (edges // 2,), generator=g)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    ei = torch.unique(torch.stack([torch.cat([src, dst]), torch.cat([dst, src])]), dim=1)
    x = (torch.rand((n, f_in), generator=g) < density).float()
    y = torch.randint(0, classes, (n,), generator=g)
    train = torch.randperm(n, generator=g)[:n_train]
    return x.to(dev), ei.to(dev), y.to(dev), train.to(dev)


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["example", "cora", "arxiv"], default="example")
    ap.add_argument("--attention", action="store_true")
    ap.add_argument("--leg", choices=["loop", "trainer", "replay", "kernel"], default="loop")
    ap.add_argument("--batch-size", type=int, default=0)
    ap.add_argument("--num-neighbors", type=lambda s: [int(k) for k in s.split(",")], default=[10, 10])
    ap.add_argument("--device-batches", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r19_node_train.jsonl"), help="the file the line is appended to")
    args = ap.parse_args()
    if args.leg == "replay" and args.batch_size:
        ap.error("a replay is the step of the full graph")
    root = os.path.abspath(args.tree)
    sys.path.insert(0, root)
    from sgracex1_amd import config, sgrace

    dev = torch.device("cuda")
    config.acc, config.accb, config.compute_attention, config.float_type = 1, 0, int(args.attention), np.float32
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.device = 32, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(1)
    if args.graph == "example":
        sys.path.insert(0, os.path.join(HERE, "examples"))
        import sgrace_node_classification as ex
        x, ei, y = ex.planted_partition(3000, 5, 200, 0.02, 0.002, 1, dev)
        train, classes = torch.randperm(3000, generator=torch.Generator().manual_seed(1)).to(dev)[:600], 5
    elif args.graph == "cora":
        x, ei, y, train = random_graph(2708, 1433, 7, 10556, 140, 0.0127, 1, dev)
        classes = 7
    else:
        x, ei, y, train = random_graph(169343, 128, 40, 2500000, 90941, 1.0, 1, dev)
        x, classes = torch.rand_like(x), 40
    n = x.shape[0]
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask[train] = True
    rec = {"graph": args.graph, "nodes": n, "edges": int(ei.shape[1]), "features": int(x.shape[1]), "classes": classes,
           "train_rows": int(train.numel()), "attention": int(args.attention), "leg": args.leg, "batch_size": args.batch_size,
           "device_batches": int(args.device_batches), "tree": "this" if root == HERE else os.path.basename(root), "tag": args.tag}

    def timed(fn):
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
        return float(np.median(out)), [round(v, 4) for v in out]

    if args.leg == "kernel":
        from sgracex1_amd import _lib, ops
        P = 16
        H = torch.rand((n, P), device=dev) - 0.5
        W, b = torch.rand((classes, P), device=dev) - 0.5, torch.zeros(classes, device=dev)
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        rec["call_ms"], rec["call_ms_trials"] = timed(lambda: ops.node_loss(H, W, b, y, mask=mask, p=0.5, seed=1, step_dev=t))
        R = _lib.SGX_NODE_LOSS_ROWS
        blocks = torch.nn.functional.pad(mask, (0, (-n) % R)).view(-1, R).any(1)
        rows_read = int(min(n, int(blocks.sum()) * R))
        rec["P"], rec["bytes"] = P, (rows_read + n) * P * 4
        rec["gb_per_s"] = rec["bytes"] / rec["call_ms"] / 1e6
        emit(rec, args.out)
        return

    net = sgrace.GAT_PYNQ(x.shape[1], 16, 1, classes).to(dev).train()
    loader = None
    if args.batch_size:
        from sgracex1_amd import pyg_lite
        data = pyg_lite.NodeData(x, ei, y, train_mask=mask)
        ready = {"prepare": "sym_norm2", "transposed": bool(args.attention)} if args.device_batches else {}
        loader = pyg_lite.NeighborLoader(data, args.num_neighbors, batch_size=args.batch_size, input_nodes=mask, shuffle=True, seed=1,
                                         **ready)
    if args.leg == "loop":
        opt = torch.optim.Adam(net.parameters(), lr=0.01, weight_decay=5e-4)
        crit = torch.nn.CrossEntropyLoss()

        def full():
            opt.zero_grad()
            loss = crit(net(x, ei)[train], y[train])
            loss.backward()
            opt.step()

        def batch_step(b):
            opt.zero_grad()
            if args.device_batches:
                loss = crit(net(b.x, b.edge_index_agg)[:b.batch_size], b.y[:b.batch_size])
            else:
                out = net(b.x, b.edge_index.flip(0))
                loss = crit(out[b.train_mask], b.y[b.train_mask])
            loss.backward()
            opt.step()
    else:
        from sgracex1_amd.train import NodeTrainer
        trainer = NodeTrainer(net, lr=0.01, weight_decay=5e-4)
        full = lambda: trainer.step(x, ei, y, mask=mask)

        def batch_step(b):
            if args.device_batches:
                trainer.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size)
            else:
                trainer.step(b.x, b.edge_index.flip(0), b.y, mask=b.train_mask)

    if loader is not None:
        def epoch():
            k = 0
            for b in loader:
                batch_step(b)
                k += 1
            return k
        epoch()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.trials):
            t0 = time.perf_counter()
            k = epoch()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / k * 1e3)
        rec["step_ms"], rec["step_ms_trials"] = float(np.median(out)), [round(v, 4) for v in out]
    else:
        fn = full
        if args.leg == "replay":
            try:
                fn = trainer.capture(x, ei, y, mask)
            except RuntimeError as e:
                rec["captured"], rec["error"] = 0, str(e)[:300]
                emit(rec, args.out)
                return
            rec["captured"] = 1
        rec["step_ms"], rec["step_ms_trials"] = timed(fn)
    emit(rec, args.out)


if __name__ == "__main__":
    main()
