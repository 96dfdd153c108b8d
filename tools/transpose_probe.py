#!/usr/bin/env python3
"""What a CSR transpose costs: ops.csr_transpose(method="device") (sgx_csr_transpose, csrc/csr_transpose.hip) against
method="torch" (the int64 key, argsort and gathers it was before), wall time per call with the stream synchronised, on
the matrices the backward transposes:

    the example's batch (3 000-node planted partition, batch 128, [10, 10]): adjacency and feature CSR
    the ogbn-products-shape batch (2.45 M nodes, 122 M edges, batch 1024, [15, 10, 5]): adjacency and feature CSR
    the ogbn-arxiv-shape adjacency (169 343 nodes, 1.17 M edges), uniform and R-MAT
    a MUTAG-shape feature matrix (one-hot, 7 columns, 18 nodes a graph) at batch 64 and 4 096

Both methods take their turn in every window (interleaved), 7 windows of 30 calls after a warm-up; the median of the
windows with their minimum and maximum.  Both include the plan a transposed feature matrix builds (nnz >= 64 rows; one
read-back, the same in both).  The outputs are checked equal first.  One JSON line per matrix; the last line applies the
rule for ops.CSR_TRANSPOSE_DEFAULT: "device" only if on no matrix its median is above the torch median by more than the
larger of the two min-max spreads.

    python tools/transpose_probe.py > profiles/r11_csr_transpose.jsonl        [--quick: 2 windows of 5, no products shape]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgracex1_amd import graphs, ops, pyg_lite  # noqa: E402

DEV = torch.device("cuda")


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def measure(name, A, windows, reps):
    forms = {m: (lambda m=m: ops.csr_transpose(A, method=m)) for m in ("device", "torch")}
    Td, od = ops.csr_transpose(A, return_order=True, method="device")
    Tt, ot = ops.csr_transpose(A, return_order=True, method="torch")
    equal = bool(torch.equal(Td.rowptr, Tt.rowptr) and torch.equal(Td.col, Tt.col) and torch.equal(od, ot)
                 and torch.equal(Td.val.view(torch.int32), Tt.val.view(torch.int32)))
    for fn in forms.values():
        for _ in range(5):
            fn()
    times = {m: [] for m in forms}
    for _ in range(windows):
        for m, fn in forms.items():
            times[m].append(window(fn, reps))
    rec = {"matrix": name, "n_rows": A.n_rows, "n_cols": A.n_cols, "nnz": A.nnz, "plan_built": Td._plan is not None,
           "equal": equal, "windows": windows, "calls_per_window": reps}
    for m, v in times.items():
        rec[m + "_ms_median"], rec[m + "_ms_min"], rec[m + "_ms_max"] = (round(statistics.median(v), 4), round(min(v), 4),
                                                                          round(max(v), 4))
    spread = max(rec["device_ms_max"] - rec["device_ms_min"], rec["torch_ms_max"] - rec["torch_ms_min"])
    rec["speedup"] = round(rec["torch_ms_median"] / rec["device_ms_median"], 2)
    rec["device_not_slower"] = bool(rec["device_ms_median"] <= rec["torch_ms_median"] + spread)
    print(json.dumps(rec), flush=True)
    return rec


def batch_of(x, ei, y, train, bs, fan):
    ld = pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y, train_mask=train), fan, batch_size=bs, input_nodes=train,
                                 shuffle=True, seed=1, prepare="sym_norm2")
    b = next(iter(ld))
    return b.adj_norm, ops.recorded(b.x, ("fea_csr", torch.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    windows, reps = (2, 5) if a.quick else (7, 30)
    recs = []
    spec = importlib.util.spec_from_file_location("nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, ei, y = mod.planted_partition(3000, 5, 200, 0.02, 0.002, 1, DEV)
    train = torch.zeros(3000, dtype=torch.bool, device=DEV)
    train[:600] = True
    adj, fea = batch_of(x, ei, y, train, 128, [10, 10])
    recs.append(measure("example batch adjacency (batch 128, [10, 10])", adj, windows, reps))
    recs.append(measure("example batch features", fea, windows, reps))
    for n_graphs in (64, 4096):
        n = 18 * n_graphs
        g = torch.Generator(device=DEV).manual_seed(n_graphs)
        # (MUTAG's node labels: mostly carbon, then nitrogen and oxygen, a few halogens)
        label = torch.multinomial(torch.tensor([0.72, 0.10, 0.15, 0.01, 0.01, 0.005, 0.005], device=DEV), n, True, generator=g)
        X = ops.Csr(torch.arange(n + 1, dtype=torch.int32, device=DEV), label.to(torch.int32).contiguous(),
                    torch.ones(n, dtype=torch.float32, device=DEV), 7)
        recs.append(measure(f"MUTAG-shape features, batch {n_graphs}", X, windows, reps))
    A = graphs.uniform_graph(169_343, 1_166_243, dtype=torch.float32)
    recs.append(measure("ogbn-arxiv shape adjacency, uniform", A, windows, reps))
    A = graphs.rmat_graph_n(169_343, 1_166_243, dtype=torch.float32)
    recs.append(measure("ogbn-arxiv shape adjacency, R-MAT", A, windows, reps))
    del A
    if not a.quick:
        n, f = 2_450_000, 100
        A = graphs.uniform_graph(n, 122_000_000, dtype=torch.float32, normalize=False)
        row = torch.repeat_interleave(torch.arange(n, device=DEV), (A.rowptr[1:] - A.rowptr[:-1]).long(), output_size=A.nnz)
        ei = torch.stack([A.col[:A.nnz].long(), row])
        del A, row
        g = torch.Generator(device=DEV).manual_seed(1)
        x = (torch.rand((n, f), device=DEV, generator=g) < 0.1).float() * torch.rand((n, f), device=DEV, generator=g)
        y = torch.randint(0, 5, (n,), device=DEV, generator=g)
        train = torch.zeros(n, dtype=torch.bool, device=DEV)
        train[torch.randperm(n, device=DEV, generator=g)[:200_000]] = True
        adj, fea = batch_of(x, ei, y, train, 1024, [15, 10, 5])
        del ei
        torch.cuda.empty_cache()
        recs.append(measure("products-shape batch adjacency (batch 1024, [15, 10, 5])", adj, windows, max(reps // 3, 3)))
        recs.append(measure("products-shape batch features", fea, windows, max(reps // 3, 3)))
    losing = [r["matrix"] for r in recs if not r["device_not_slower"]]
    print(json.dumps({"rule": "device is the default only if it is not slower on every matrix", "all_equal": all(r["equal"] for r in recs),
                      "losing_matrices": losing, "default": "device" if not losing else "torch"}), flush=True)


if __name__ == "__main__":
    main()
