#!/usr/bin/env python3
"""The evaluation pass of a node classifier over neighbour-sampled batches (profiles/r23_node_eval.jsonl): the example's
graph (3 000 nodes, its 2 400 nodes outside the training set) at batch 128 and [10, 10], GCN and attention.  Two legs:

  eager   NodeTrainer.evaluate per batch of the prepared loader, the counts read back per batch and summed on the host
          (what a pass was before sgx_node_eval; runs on a checkout without it too: --legs eager)
  replay  NodeTrainer.capture_eval_loader's pass over the padded loader and one EvalSums.read

    python tools/node_eval_probe.py [--legs eager,replay] [--runs 3] [--label TEXT]

The legs alternate, --runs windows each (three at least); one JSON line per model and leg."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="eager,replay")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5, help="passes per window")
    ap.add_argument("--label", default=None, help="a tag printed with the run (which checkout this is)")
    a = ap.parse_args()
    legs, runs = a.legs.split(","), max(3, a.runs)
    from sgracex1_amd import config, pyg_lite, sgrace
    from sgracex1_amd import train
    dev = torch.device("cuda")
    spec = importlib.util.spec_from_file_location("nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n, bs, fan = 3000, 128, [10, 10]
    x, ei, y = mod.planted_partition(n, 5, 200, 0.02, 0.002, 1, dev)
    nodes = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)[n // 5:]
    data = pyg_lite.NodeData(x, ei, y)
    if a.label:
        print(json.dumps({"label": a.label}), flush=True)
    for attention in (0, 1):
        config.acc, config.accb, config.device, config.compute_attention, config.gat_edge_outputs = 1, 0, "cuda", attention, 1
        sgrace.init_SGRACE()
        torch.manual_seed(0)
        model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(dev).train()
        trainer = train.NodeTrainer(model, lr=0.01)
        kw = dict(batch_size=bs, input_nodes=nodes, shuffle=False, seed=1, prepare="sym_norm2")
        run, result = {}, {}
        if "eager" in legs:
            plain = pyg_lite.NeighborLoader(data, fan, **kw)

            def eager_pass():
                rows = hits = 0
                loss = 0.0
                for b in plain:
                    counts, mean = trainer.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size)
                    m, h = counts.tolist()                           # the read-back of every batch
                    rows, hits, loss = rows + m, hits + h, loss + float(mean) * m
                return rows, hits, loss

            run["eager"] = eager_pass
        if "replay" in legs:
            padded = pyg_lite.NeighborLoader(data, fan, pad=True, **kw)
            captured = trainer.capture_eval_loader(padded)

            def replay_pass():
                return train.EvalSums.read(captured())[0]            # the pass's one read-back

            run["replay"] = replay_pass
        times = {leg: [] for leg in run}
        for leg in run:                                              # warm-up: the caches, the workspaces, the allocator
            for _ in range(2):
                result[leg] = run[leg]()
        torch.cuda.synchronize()
        for _ in range(runs):
            for leg in run:                                          # the legs take turns
                t0 = time.perf_counter()
                for _ in range(a.passes):
                    result[leg] = run[leg]()
                torch.cuda.synchronize()
                times[leg].append((time.perf_counter() - t0) / a.passes * 1e3)
        if "replay" in legs:
            padded.status()
        for leg in run:
            rows, hits, loss = result[leg]
            print(json.dumps({"measure": "evaluation pass over a NeighborLoader (sample + preparation + layers + head + sums)",
                              "leg": leg, "model": "GAT" if attention else "GCN", "graph": "example (3 000 nodes)",
                              "eval_nodes": int(nodes.numel()), "batch": bs, "fanouts": fan, "batches_per_pass": -(-int(nodes.numel()) // bs),
                              "read_backs_per_pass": -(-int(nodes.numel()) // bs) if leg == "eager" else 1,
                              "pass_ms_median": round(statistics.median(times[leg]), 4), "pass_ms_min": round(min(times[leg]), 4),
                              "pass_ms_max": round(max(times[leg]), 4), "windows": runs, "passes_per_window": a.passes,
                              "rows": rows, "hits": hits, "loss_sum": loss}), flush=True)


if __name__ == "__main__":
    main()
