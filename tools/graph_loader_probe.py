#!/usr/bin/env python3
"""What a shuffled training step costs with the batches collated on the host (pyg_lite.DataLoader: Python collate,
host-to-device copies, then the synchronising builders -- graph_ptr_of, csr_from_edge_index, the feature CSR, the batch
plan) against the device collator (pyg_lite.GraphLoader: one sgx_collate_graphs launch, attached CSRs, trusted plans).

Workloads, MOL cell 18's model (7 -> 64 ReLU -> 64, mean pool, dropout, 64 -> 2 head, cross entropy, Adam) with
GCN_PYNQ(train_stack=True), layer_count 2, fp16 layers:
  step    MUTAG (188 graphs) at batch 256 (the notebook's; one shuffled batch per epoch) and 64; and the million-graph MUTAG
          replica of tools/stack_train_probe.py at batch 4096.  step_ms = host wall clock of whole steps (loader
          iteration, forward, loss, backward, Adam), the window closed by a device synchronisation, after three warm-up
          steps; per loader.  cached: the same batch every step (the loop of examples/molecule_gcn_train.py), for reference.
  collate sgx_collate_graphs alone on a prepared batch (hipEvents around --reps launches), and with GraphSet.prepare
          (host offsets and the pinned upload) included: graphs/s, and GB/s over the bytes the kernel must move.
  --model gat [--quant 8]: the shuffled GAT_POOL_PYNQ(train_stack=True) step (fp32 layers, layer_count 2; quantised at N
          bits under --quant) on MUTAG at batch 64 and on the million-graph replica at batch 4096, through the plain
          GraphLoader (the model normalises, quantises and reads the dead-row flag back per batch) and the prepared one
          (GraphLoader(prepare="sym_norm2", quant=): everything gathered by the collation launch); and the collation alone
          without and with the extras.  --leg plain runs the plain leg alone (it uses nothing a tree without the prepared
          loader lacks).
  --only replay [--model gat] [--replay-leg eager|replay] [--big] [--pad-rows N]: the shuffled epoch through
          train.StackTrainer -- eager: trainer.step over the plain (gat: prepared) GraphLoader's batches, which runs on a
          tree without padded batches too; replay: StackTrainer.capture_loader over GraphLoader(pad=True), one recorded
          step for every full batch -- on MUTAG at batch 64, or with --big on the million-graph replica at batch 4096.
          step_ms = host wall clock of whole epochs over their steps, closed by a synchronisation, after one warm-up
          epoch; the replay line also gives the padding overhead N over the mean n.  --model gat --quant 8
          [--attention 0]: the quantised step (GCN layers with --attention 0) -- eager over GraphLoader(prepare=
          "sym_norm2", quant=), which a tree without padded quantised batches runs too; replay over the same loader with
          pad=True, pad_quant=True.
One JSON line each.  --stats CSV turns a `rocprofv3 --kernel-trace --stats` kernel_stats file of a `--only collate` run
into one line for the collate kernel.

    python tools/graph_loader_probe.py > profiles/r06_graph_loader.jsonl
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgracex1_amd import molecule_gcn as M, ops, pyg_lite as G, pynq_shim  # noqa: E402


def mutag_graphs():
    raw = np.load(os.path.join(ROOT, "tests", "golden", "mutag_raw.npz"))
    return G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])


def model(dev):
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2
    return M.GCN_PYNQ(64, 7, 2, ip, train_stack=True).to(dev).train()


def step_times(graphs, batch_size, dev, max_steps, which):
    """{loader: per-step ms} over up to max_steps steps after a warm-up of a few steps."""
    out = {}
    crit = torch.nn.CrossEntropyLoss()
    for name in which:
        torch.manual_seed(5)
        m = model(dev)
        opt = torch.optim.Adam(m.parameters(), lr=0.01)
        gen = torch.Generator().manual_seed(12345)
        if name == "host":
            loader = G.DataLoader(graphs, batch_size=batch_size, shuffle=True, generator=gen)
        elif name == "device":
            loader = G.GraphLoader(graphs, batch_size=batch_size, shuffle=True, generator=gen, device=dev)
        else:                                                            # cached: one batch, the same tensors every step
            fixed = G.collate(graphs[:batch_size]).to(dev)
            loader = [fixed] * len(G.DataLoader(graphs, batch_size=batch_size))

        def batches():
            while True:
                for b in loader:
                    yield b.to(dev) if name == "host" else b

        it = batches()

        def run(n):
            for _ in range(n):
                b = next(it)
                opt.zero_grad()
                crit(m(1, b.x, b.edge_index, b.batch), b.y).backward()
                opt.step()

        run(min(3, max_steps))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(max_steps)
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) * 1e3 / max_steps
        del m, opt, loader
    return out


def gat_model(dev, qbits, attention=1):
    from sgracex1_amd import config, sgrace
    config.acc, config.compute_attention, config.float_type = 1, int(attention), np.float32
    config.fake_quantization, config.w_qbits = int(qbits is not None), qbits or 8
    sgrace.init_SGRACE().register_map.layer_count = 2
    return sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(dev).train(), sgrace.quant_constants


def gat_step_times(gs, batch_size, dev, max_steps, qbits, legs):
    """{leg: per-step ms} of the shuffled train_stack step of the attention model; the plain leg first, on the set as
    uploaded (prepare_sym_norm2 adds to it)."""
    out = {}
    crit = torch.nn.CrossEntropyLoss()
    for name in legs:
        torch.manual_seed(5)
        m, qc = gat_model(dev, qbits)
        opt = torch.optim.Adam(m.parameters(), lr=0.01)
        gen = torch.Generator().manual_seed(12345)
        kw = dict(prepare="sym_norm2", quant=qc) if name == "prepared" else {}
        loader = G.GraphLoader(gs, batch_size=batch_size, shuffle=True, generator=gen, device=dev, dtypes=(torch.float32,), **kw)

        def batches():
            while True:
                for b in loader:
                    yield b

        it = batches()

        def run(n):
            for _ in range(n):
                b = next(it)
                opt.zero_grad()
                crit(m(b.x, b.edge_index, b.batch), b.y).backward()
                opt.step()

        run(min(3, max_steps))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(max_steps)
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) * 1e3 / max_steps
        del m, opt, loader
    return out


def gat_lines(gs, name, batch_size, dev, args):
    legs = ("plain", "prepared") if args.leg == "both" else (args.leg,)
    if "plain" not in legs or not hasattr(gs, "prepare_sym_norm2"):
        plain_collate = None
    else:
        plain_collate = collate_times(gs, batch_size, args.reps, args.trials, dtypes=(torch.float32,))["collate_ms"]
    t = gat_step_times(gs, batch_size, dev, args.steps, args.quant, legs)
    line = {"workload": f"{name}_gat_train_stack", "graphs": len(gs), "batch_size": batch_size, "quant": args.quant,
            "steps": args.steps, **{f"step_ms_{k}_loader": v for k, v in t.items()}}
    if len(t) == 2:
        line["plain_over_prepared"] = t["plain"] / t["prepared"]
    print(json.dumps(line), flush=True)
    if "prepared" in legs:
        from sgracex1_amd import sgrace
        extras = gs.prepare_sym_norm2((torch.float32,), sgrace.quant_constants)
        c = collate_times(gs, batch_size, args.reps, args.trials, dtypes=(torch.float32,), extras=extras)
        print(json.dumps({"workload": f"collate_{name}_gat", "quant": args.quant, "graphs": c["graphs"], "rows": c["rows"],
                          "norm_entries": c["norm_entries"], "extras": 1 + len(extras.keys),
                          "collate_ms_plain": plain_collate, "collate_ms_extras": c["collate_ms"],
                          "prepare_and_collate_wall_ms_extras": c["prepare_and_collate_wall_ms"]}), flush=True)


def replay_line(graphs, name, batch_size, dev, args):
    """One line: the shuffled epoch's step through StackTrainer, eager on unpadded batches or replayed on padded ones."""
    from sgracex1_amd import train
    torch.manual_seed(5)
    gat = args.model == "gat"
    m, qc = gat_model(dev, args.quant, args.attention) if gat else (model(dev), None)
    kw = dict(dtypes=(torch.float32,), prepare="sym_norm2") if gat else {}
    if qc is not None:
        kw.update(quant=qc)                        # the quantised step: the prepared quantised loader in both legs
    gs = ops.GraphSet(graphs, dev)
    replay = args.replay_leg == "replay"
    if replay:
        kw.update(pad=True, pad_rows=args.pad_rows, **({} if qc is None else {"pad_quant": True}))
    loader = G.GraphLoader(gs, batch_size=batch_size, shuffle=True, generator=torch.Generator().manual_seed(12345), **kw)
    trainer = train.StackTrainer(m, lr=0.01)
    line = {"workload": f"{name}_{args.model}_trainer_epoch", "leg": args.replay_leg, "graphs": len(gs), "batch_size": batch_size}
    if gat:
        line.update(quant=args.quant, attention=args.attention)
    if replay:
        epoch = trainer.capture_loader(loader)
        cap = loader.capacity
        padded = [loader.padded(ids) for ids in loader.batches()]
        line.update(pad_rows=cap.n_rows, pad_graphs=cap.n_graphs, filler_rows=cap.filler_rows,
                    rows_over_mean_rows=cap.n_rows / (float(np.mean(gs.counts[0])) * batch_size),
                    padded_batches_of_an_epoch=f"{sum(padded)} of {len(padded)}")
    else:
        def epoch():
            return [trainer.step(b.x, b.edge_index, b.batch, b.y) for b in loader]
    epochs = max(1, args.steps // len(loader))
    epoch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        steps = len(epoch())
    torch.cuda.synchronize()
    line.update(epochs=epochs, steps_per_epoch=steps, step_ms=(time.perf_counter() - t0) * 1e3 / (epochs * steps),
                fused_steps=trainer.fused_steps)
    print(json.dumps(line), flush=True)


def collate_bytes(gs, index):
    """Bytes sgx_collate_graphs must read and write for a batch (fp16 CSR values out)."""
    n, E, na, nf, B, F = index.n_rows, index.n_edges, index.nnz_adj, index.nnz_fea, index.n_graphs, gs.n_feat
    read = n * F * 4 + 2 * E * 4 + 2 * (n * 4 + na * 8) + (nf * 8) + B * (4 * 4 + 5 * 4 + 8)
    write = n * F * 4 + 2 * E * 8 + n * 8 + B * 8 + (B + 1) * 4 + 2 * (n + 1) * 4 + na * 6 + nf * 6
    return read + write


def collate_times(gs, batch_size, reps, trials, seed=3, dtypes=(torch.float16,), extras=None):
    perm = torch.randperm(len(gs), generator=torch.Generator().manual_seed(seed)).numpy()[:batch_size]
    index = gs.prepare(perm)
    kw = {} if extras is None else {"extras": extras}
    out = ops.collate_graphs(gs, index, dtypes, **kw)

    def timed(fn):
        res = []
        for _ in range(trials):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            res.append((a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3 / reps))
        return [float(np.median([r[k] for r in res])) for k in range(2)]

    kernel_ms, _ = timed(lambda: ops.collate_graphs(gs, index, dtypes, out=out, **kw))
    _, prepared_ms = timed(lambda: ops.collate_graphs(gs, perm, dtypes, out=out, **kw))
    nbytes = collate_bytes(gs, index)                       # (the batch's own bytes, fp16 values: the extras are not counted)
    return {"graphs": int(index.n_graphs), "norm_entries": getattr(index, "nnz_norm", None), "rows": index.n_rows, "edges": index.n_edges, "adj_entries": index.nnz_adj,
            "fea_entries": index.nnz_fea, "bytes": nbytes, "collate_ms": kernel_ms,
            "collate_graphs_per_s": index.n_graphs / (kernel_ms * 1e-3), "collate_GBps": nbytes / (kernel_ms * 1e-3) / 1e9,
            "prepare_and_collate_wall_ms": prepared_ms,
            "prepare_and_collate_graphs_per_s": index.n_graphs / (prepared_ms * 1e-3)}


def stats_line(path):
    with open(path) as f:
        for row in csv.DictReader(f):
            if "collate_graphs_kernel" in row["Name"]:
                return {"workload": "rocprofv3_kernel_stats", "kernel": "collate_graphs_kernel", "calls": int(row["Calls"]),
                        "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                        "max_us": float(row["MaxNs"]) / 1e3, "source": os.path.basename(path)}
    raise SystemExit(f"no collate kernel in {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["step", "big", "collate", "replay"], default=None)
    ap.add_argument("--replay-leg", choices=["eager", "replay"], default="replay")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--pad-rows", type=int, default=None)
    ap.add_argument("--copies", type=int, default=5320)          # 5320 x 188 = 1,000,160 graphs
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--big-steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--model", choices=["gcn", "gat"], default="gcn")
    ap.add_argument("--quant", type=int, default=None, choices=[8, 4, 2, 1])
    ap.add_argument("--attention", type=int, default=1, choices=[0, 1])      # --only replay --model gat: 0 = GCN layers
    ap.add_argument("--leg", choices=["both", "plain", "prepared"], default="both")
    args = ap.parse_args()
    if args.quant is not None and args.model != "gat":
        ap.error("--quant times the quantised attention layers: --model gat")
    if args.stats is not None:
        if not os.path.isfile(args.stats):
            raise SystemExit(f"--stats: no such file {args.stats!r}")
        print(json.dumps(stats_line(args.stats)), flush=True)
        return
    dev = torch.device("cuda")
    graphs = mutag_graphs()
    if args.only == "replay":
        if args.big:
            replay_line(graphs * args.copies, "mutag_replica", 4096, dev, args)
        else:
            replay_line(graphs, "mutag", 64, dev, args)
        return
    if args.model == "gat":
        if args.only in (None, "step"):
            gat_lines(ops.GraphSet(graphs, dev), "mutag", 64, dev, args)
        if args.only in (None, "big"):
            gat_lines(ops.GraphSet(graphs * args.copies, dev), "mutag_replica", 4096, dev, args)
        return
    if args.only in (None, "step"):
        for bs in (256, 64):
            t = step_times(graphs, bs, dev, args.steps, ("cached", "host", "device"))
            print(json.dumps({"workload": "mutag_train_stack", "graphs": len(graphs), "batch_size": bs,
                              "step_ms_cached_batch": t["cached"], "step_ms_host_loader": t["host"],
                              "step_ms_device_loader": t["device"], "host_over_device": t["host"] / t["device"]}), flush=True)
    if args.only in (None, "collate"):
        gs = ops.GraphSet(graphs, dev)
        for bs in (64, 188):
            print(json.dumps({"workload": "collate_mutag", **collate_times(gs, bs, args.reps, args.trials)}), flush=True)
    if args.only in (None, "big", "collate"):
        big = graphs * args.copies
        t0 = time.perf_counter()
        gs = ops.GraphSet(big, dev)
        torch.cuda.synchronize()
        upload_s = time.perf_counter() - t0
        print(json.dumps({"workload": "collate_mutag_replica", "dataset_graphs": len(big), "upload_s": upload_s,
                          **collate_times(gs, 4096, args.reps, args.trials)}), flush=True)
        if args.only != "collate":
            t = {}
            for name, steps in (("host", args.big_steps), ("device", args.steps)):
                t.update(step_times(big if name == "host" else gs, 4096, dev, steps, (name,)))
            print(json.dumps({"workload": "mutag_replica_train_stack", "graphs": len(big), "batch_size": 4096,
                              "step_ms_host_loader": t["host"], "step_ms_device_loader": t["device"],
                              "host_steps": args.big_steps, "device_steps": args.steps,
                              "host_over_device": t["host"] / t["device"]}), flush=True)


if __name__ == "__main__":
    main()
