"""What one epoch's evaluation of examples/molecule_gcn_train.py costs (the MUTAG train set of 188 graphs and test set of
50), three ways, host wall clock with the read-back of the results inside the timed region:

    --mode torch    the notebook's accuracy(): the model's eval forward, argmax, ==, mean and float() per set
    --mode eager    StackTrainer.evaluate per set, both sets' counts read back in one transfer
    --mode replay   StackTrainer.capture_eval_loader over unshuffled padded loaders at --batch-size, one transfer

One mode per process (a fresh allocator, fresh caches); prints one JSON line.  Run each mode at least twice: the spread
between two processes of one mode is what a difference between modes is held against.

    python tools/eval_probe.py --mode replay --model gcn [--batch-size 64] [--reps 200] [--out profiles/r21_stack_eval.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sgracex1_amd import molecule_gcn as M, pyg_lite as G, pynq_shim  # noqa: E402
from sgracex1_amd.train import EvalSums, StackTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["torch", "eager", "replay"], required=True)
    ap.add_argument("--model", choices=["gcn", "gat"], default="gcn")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    raw = np.load(os.path.join(ROOT, "tests", "golden", "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    torch.manual_seed(12345)
    graphs = [graphs[i] for i in torch.randperm(len(graphs)).tolist()]
    sets = (graphs, graphs[50:100])
    whole = [G.collate(s).to(dev) for s in sets]
    prepared = {}
    if args.model == "gat":
        from sgracex1_amd import config, sgrace
        config.acc, config.compute_attention = 1, 1
        sgrace.init_SGRACE().register_map.layer_count = 2
        torch.manual_seed(12345)
        model = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(dev)
        forward = lambda b: model(b.x, b.edge_index, b.batch)
        prepared = dict(dtypes=(sgrace._torch_dtype(),), prepare="sym_norm2")
    else:
        ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
        ip.register_map.layer_count = 2
        model = M.GCN_PYNQ(64, 7, 2, ip, train_stack=True).to(dev)
        forward = lambda b: model(1, b.x, b.edge_index, b.batch)
    trainer = StackTrainer(model, lr=0.01)
    for _ in range(5):                                                   # a few steps: the state of a loop in progress
        trainer.step(whole[0].x, whole[0].edge_index, whole[0].batch, whole[0].y)
    model.train()

    if args.mode == "torch":
        def evaluate():
            out = []
            for b in whole:
                model.eval()
                with torch.no_grad():
                    pred = forward(b).argmax(dim=1)
                out.append(float((pred == b.y).float().mean()))
            model.train()
            return out
    elif args.mode == "eager":
        sums = [EvalSums(dev), EvalSums(dev)]

        def evaluate():
            for b, into in zip(whole, sums):
                trainer.evaluate(b.x, b.edge_index, b.batch, b.y, into=into.zero_())
            return [float(np.float32(h) / np.float32(n)) for n, h, _ in EvalSums.read(*sums)]
    else:
        passes = [trainer.capture_eval_loader(G.GraphLoader(s, batch_size=args.batch_size, shuffle=False, device=dev, pad=True,
                                                            **prepared)) for s in sets]

        def evaluate():
            for run_pass in passes:
                run_pass()
            return [float(np.float32(h) / np.float32(n)) for n, h, _ in EvalSums.read(*[p.sums for p in passes])]

    for _ in range(args.warmup):
        acc = evaluate()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        acc = evaluate()                                                 # ends in its read-back: the device is idle again
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    line = {"probe": "stack_eval", "mode": args.mode, "model": args.model, "batch_size": args.batch_size if args.mode == "replay" else 0,
            "reps": args.reps, "eval_ms_median": round(statistics.median(times), 4), "eval_ms_min": round(times[0], 4),
            "eval_ms_p90": round(times[int(0.9 * len(times))], 4), "train_acc": round(acc[0], 4), "test_acc": round(acc[1], 4),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
