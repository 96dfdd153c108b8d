#!/usr/bin/env python3
"""The entry-split aggregation (ops.spmm(..., schedule="flat"), sgx_spmm_csr_flat) beside the planned and the unplanned
ops.spmm, interleaved in one process, three rounds of (best, median) ms each; one JSON line per leg:

    arxiv-rmat, arxiv   the R-MAT and the uniform graph of ogbn-arxiv's size (169 343 rows, 2.33 M entries), 256 fp16 columns
    node-batch-xt       X^T of the node example's padded batch (NeighborLoader(pad=True) on its planted-partition graph,
                        --nodes / --batch-size / fan-out 10) times a [rows, --hidden] fp32 gradient: one feature column
                        that many rows share is one long row of X^T

    python3 tools/spmm_flat_probe.py [--nodes 3000] [--batch-size 512] [--hidden 16] > profiles/r28_spmm_flat.jsonl

Every leg also checks the flat result against the planned one within the fp32-sum bound of tests/_spmm_acc_ref.py's kind
(a relative 2^-9 on fp16 stores here: a probe's sanity check, the tests hold the derived bound)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from sgracex1_amd import graphs, ops  # noqa: E402
from sgracex1_amd.hipevents import Event  # noqa: E402


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    ts = []
    for _ in range(iters):
        b, e = Event(), Event()
        b.record(s)
        fn()
        e.record(s)
        ts.append(b.elapsed_ms(e))
    ts.sort()
    return round(ts[0], 4), round(ts[len(ts) // 2], 4)


def leg(name, A, H, relu=True):
    """A: a Csr that wants a plan (it is built here, outside the timing)"""
    D = torch.empty((A.n_rows, H.shape[1]), dtype=H.dtype, device=H.device)
    A.plan
    deg = (A.rowptr[1:] - A.rowptr[:-1])
    rec = {"leg": name, "rows": A.n_rows, "entries": A.nnz, "longest_row": int(deg.max()), "columns": H.shape[1],
           "dtype": str(H.dtype).replace("torch.", ""), "plan_long_rows": A.plan.long_rows, "plan_reordered": A.plan.reordered}
    forms = {"planned": lambda: ops.spmm(A, H, relu=relu, out=D), "unplanned": lambda: ops.spmm(A, H, relu=relu, out=D, use_plan=False),
             "flat": lambda: ops.spmm(A, H, relu=relu, out=D, schedule="flat")}
    for _ in range(3):
        for form, fn in forms.items():
            rec.setdefault("ms_" + form, []).append(timed(fn))
    forms["planned"]()
    want = D.float().clone()
    forms["flat"]()
    err = ((D.float() - want).abs() / want.abs().clamp_min(1e-3)).max().item()
    rec["flat_vs_planned_max_rel"] = round(err, 6)
    rec["agrees"] = bool(err < 2.0 ** -9)
    print(json.dumps(rec), flush=True)


def node_batch_xt(nodes, batch_size, hidden, seed=1):
    from sgrace_node_classification import planted_partition
    from sgracex1_amd import pyg_lite
    dev = torch.device("cuda")
    x, edge_index, y = planted_partition(nodes, 5, 200, 0.02, 0.002, seed, dev)
    train_mask = torch.zeros(nodes, dtype=torch.bool, device=dev)
    train_mask[torch.randperm(nodes, generator=torch.Generator().manual_seed(seed))[: max(nodes // 5, batch_size)].to(dev)] = True
    data = pyg_lite.NodeData(x, edge_index, y, train_mask=train_mask)
    loader = pyg_lite.NeighborLoader(data, [10], batch_size=batch_size, input_nodes=train_mask, shuffle=True, seed=seed,
                                     prepare="sym_norm2", pad=True, dtype=torch.float32)
    seeds, input_id, step = next(iter(loader.epoch_batches()))
    loader.load(seeds, step)
    b = loader.padded_batch(input_id)
    fea = ops.recorded(b.x, ("fea_csr", torch.float32))
    Xt = ops.csr_transpose(fea, method="device")
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    G = torch.rand((Xt.n_cols, hidden), generator=g, device=dev) - 0.5
    return Xt, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=3000)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for name, A in (("arxiv-rmat", graphs.rmat_graph_n(169_343, 2_330_000, seed=5, device=dev)),
                    ("arxiv", graphs.uniform_graph(169_343, 2_330_000, seed=5, device=dev))):
        leg(name, A, torch.rand((A.n_rows, 256), generator=g, device=dev).half())
    Xt, G = node_batch_xt(a.nodes, a.batch_size, a.hidden)
    leg("node-batch-xt", Xt, G, relu=False)


if __name__ == "__main__":
    main()
