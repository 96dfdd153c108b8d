#!/usr/bin/env python3
"""Model selection on the device (profiles/r25_keep_best.jsonl): a whole run of the node example's replayed configuration
(3 000 nodes, batch 128, [10, 10], --device-batches --trainer --replay), GCN and attention, in three legs:

  parent     the per-epoch read-back (EvalSums.read and the comparison on the host) on a checkout of the parent commit
             (--parent DIR, built; without it the leg is reported as not measured)
  readback   the same command on this checkout
  keep-best  --keep-best on this checkout: one sgx_keep_best per epoch, one read-back per run

Every run is a process of its own; the legs alternate, --runs of each (three at least).  What is timed is the example's
own ms_per_epoch (the epoch loop, synchronised at its end).  Then sgx_keep_best alone, in this process: at the example
model's parameter sizes and at 16 tensors of 1 Mi floats, for a call that wins (the copy runs) and one that does not.

    python tools/keep_best_probe.py [--parent DIR] [--epochs 60] [--runs 3]

One JSON line per model and leg, one per timed call shape."""
import argparse
import ast
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def example_run(root, attention, epochs, keep_best):
    cmd = [sys.executable, os.path.join(root, "examples", "sgrace_node_classification.py"), "--epochs", str(epochs), "--batch-size", "128",
           "--num-neighbors", "10,10", "--device-batches", "--trainer", "--replay"]
    cmd += ["--attention"] if attention else []
    cmd += ["--keep-best"] if keep_best else []
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, check=True).stdout
    return ast.literal_eval([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def time_calls(params, wins, calls=200):
    """Microseconds per ops.keep_best over `calls` calls behind a warm-up; wins: the state is put back to the fresh one
    before every call (a device copy of 32 bytes, inside the timed window of both forms), so every call copies."""
    import torch
    from sgracex1_amd import ops
    dev = params[0].device
    snapshot = [torch.empty_like(p) for p in params]
    fresh = torch.tensor([1, 0, -1, 0], dtype=torch.int64).to(dev)
    state = fresh.clone()
    sums = [torch.tensor([100, 50 if wins else 0, 0], dtype=torch.int64).to(dev)]
    log = torch.zeros((1, 3), dtype=torch.int64, device=dev)
    times = []
    for window in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            state.copy_(fresh)
            ops.keep_best(params, snapshot, sums, state, log)
        torch.cuda.synchronize()
        if window:
            times.append((time.perf_counter() - t0) / calls * 1e6)
    assert int(state[2]) == (0 if wins else -1)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    runs = max(3, a.runs)
    legs = [("parent", a.parent, False), ("readback", ROOT, False), ("keep-best", ROOT, True)]
    for attention in (0, 1):
        ms = {name: [] for name, _, _ in legs}
        last = {}
        for _ in range(runs):
            for name, root, keep_best in legs:               # the legs take turns
                if root is None:
                    continue
                last[name] = example_run(root, attention, a.epochs, keep_best)
                ms[name].append(last[name]["ms_per_epoch"])
        for name, root, keep_best in legs:
            line = {"measure": "node example, replayed mini-batch run: ms per epoch (steps, both passes, model selection)",
                    "leg": name, "model": "GAT" if attention else "GCN", "epochs": a.epochs, "runs": len(ms[name])}
            if root is None:
                line["not_measured"] = "no checkout of the parent commit was given (--parent)"
            else:
                line.update(ms_per_epoch=[round(v, 3) for v in ms[name]], median=round(statistics.median(ms[name]), 3),
                            spread=round(max(ms[name]) - min(ms[name]), 3), test_acc=last[name]["test_acc"],
                            read_backs_per_run=1 if keep_best else a.epochs)
                if keep_best:
                    line.update(best_epoch=last[name]["best_epoch"], restored_test_acc=last[name]["restored_test_acc"])
            print(json.dumps(line), flush=True)
    import torch
    from sgracex1_amd import config, sgrace
    dev = torch.device("cuda")
    config.acc, config.device, config.compute_attention = 1, "cuda", 1
    sgrace.init_SGRACE()
    model = sgrace.GAT_PYNQ(200, 16, 1, 5).to(dev)
    shapes = {"the example model's parameters": [p.detach().float().contiguous() for p in model.parameters()],
              "16 tensors of 1 Mi floats": [torch.randn(1 << 20, device=dev) for _ in range(16)]}
    for what, params in shapes.items():
        for wins in (False, True):
            t = time_calls(params, wins)
            nbytes = sum(p.numel() for p in params) * 4
            print(json.dumps({"measure": "sgx_keep_best alone (with the 32-byte state reset in front of it), microseconds per call",
                              "shape": what, "tensors": len(params), "bytes": nbytes, "wins": wins,
                              "us_per_call": [round(v, 2) for v in t], "median": round(statistics.median(t), 2),
                              **({"copy_GBps": round(2 * nbytes / statistics.median(t) / 1e3, 1)} if wins else {})}), flush=True)


if __name__ == "__main__":
    main()
