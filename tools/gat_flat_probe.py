#!/usr/bin/env python3
"""The entry-split GAT aggregate (ops.gat_aggregate(..., schedule="flat"), sgx_gat_aggregate_flat) beside the planned and the
unplanned (use_plan=False) ops.gat_aggregate, one head, interleaved in one process, three rounds of (best, median) ms of 20
launches each; one JSON line per leg:

    arxiv-rmat, arxiv   the R-MAT and the uniform graph of ogbn-arxiv's size (169 343 rows, 2.33 M entries), 256 columns,
                        fp16 and fp32
    node-batch-hub      a padded node batch of the node example at fan-outs [100, 10]: --batch-size seeds of its
                        planted-partition graph (made dense enough, --p-in / --p-out, for a seed to have 100 neighbours),
                        100 neighbours per seed, 10 per first-hop node, the seeds first, self loops, rows normalised, the
                        entry arrays padded to a capacity.  Built here with torch ops: NeighborLoader(pad=True) refuses
                        fan-outs over 63.

    python3 tools/gat_flat_probe.py [--nodes 3000] [--batch-size 512] [--hidden 64] > profiles/r29_gat_flat.jsonl

The planned and the unplanned columns run kernels this form does not touch: they are the yardstick.  Every leg also checks the
flat result against the planned one (a relative 2^-8 on fp16 stores: a probe's sanity check, the tests hold the derived bound)."""
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


def leg(name, A, Wh, att):
    """A: a Csr that wants a plan (it is built here, outside the timing)"""
    D = torch.empty((A.n_rows, Wh.shape[1]), dtype=Wh.dtype, device=Wh.device)
    planned = A.wants_plan
    if planned:
        A.gat_plan
    deg = (A.rowptr[1:] - A.rowptr[:-1])
    rec = {"leg": name, "rows": A.n_rows, "entries": int(A.rowptr[-1]), "capacity": A.nnz, "longest_row": int(deg.max()),
           "columns": Wh.shape[1], "dtype": str(Wh.dtype).replace("torch.", ""), "has_plan": bool(planned)}
    kw = dict(alpha=0.2, relu=True, fill_dead_rows=False, out=D)
    forms = {"planned": lambda: ops.gat_aggregate(A, Wh, att, **kw),
             "unplanned": lambda: ops.gat_aggregate(A, Wh, att, use_plan=False, **kw),
             "flat": lambda: ops.gat_aggregate(A, Wh, att, schedule="flat", **kw)}
    for _ in range(3):
        for form, fn in forms.items():
            rec.setdefault("ms_" + form, []).append(timed(fn))
    forms["planned"]()
    want = D.float().clone()
    forms["flat"]()
    err = ((D.float() - want).abs() / want.abs().clamp_min(1e-2)).max().item()
    rec["flat_vs_planned_max_rel"] = round(err, 6)
    rec["agrees"] = bool(err < 2.0 ** -8)
    print(json.dumps(rec), flush=True)


def node_batch_hub(nodes, batch_size, p_in, p_out, dtype, seed=1, fanouts=(100, 10), pad_to=4096):
    from sgrace_node_classification import planted_partition
    dev = torch.device("cuda")
    _, edge_index, _ = planted_partition(nodes, 5, 8, p_in, p_out, seed, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    adj = torch.zeros((nodes, nodes), dtype=torch.bool, device=dev)
    adj[edge_index[0], edge_index[1]] = True
    adj[edge_index[1], edge_index[0]] = True
    adj.fill_diagonal_(False)

    def sample(rows, k):                                  # up to k neighbours of each row, uniformly: [len(rows), nodes] bool
        score = torch.rand((rows.numel(), nodes), generator=g, device=dev).masked_fill_(~adj[rows], -1.0)
        top = score.topk(k, dim=1)
        keep = torch.zeros_like(score, dtype=torch.bool)
        keep.scatter_(1, top.indices, top.values >= 0)
        return keep

    seeds = torch.randperm(nodes, generator=g, device=dev)[:batch_size]
    hop1 = sample(seeds, fanouts[0])
    is_seed = torch.zeros(nodes, dtype=torch.bool, device=dev)
    is_seed[seeds] = True
    first = (hop1.any(0) & ~is_seed).nonzero().flatten()
    hop2 = sample(first, fanouts[1])
    reached = hop1.any(0) | hop2.any(0) | is_seed
    rest = (reached & ~is_seed).nonzero().flatten()
    rest = torch.cat([first, rest[~torch.isin(rest, first)]])
    order = torch.cat([seeds, rest])                      # local id -> global id, the seeds first
    local = torch.full((nodes,), -1, dtype=torch.int64, device=dev)
    local[order] = torch.arange(order.numel(), device=dev)
    n = order.numel()
    M = torch.zeros((n, n), dtype=torch.bool, device=dev)
    M[:batch_size] = hop1[:, order]
    M[batch_size:batch_size + first.numel()] = hop2[:, order]
    M.fill_diagonal_(True)
    deg = M.sum(1)
    row, col = M.nonzero(as_tuple=True)
    val = (1.0 / deg[row].float()).to(dtype)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = deg.cumsum(0)
    cap = -(-row.numel() // pad_to) * pad_to
    col_p = torch.zeros(cap, dtype=torch.int32, device=dev)
    val_p = torch.zeros(cap, dtype=dtype, device=dev)
    col_p[:col.numel()], val_p[:col.numel()] = col.to(torch.int32), val
    return ops.Csr(rowptr, col_p, val_p, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=3000)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--p-in", type=float, default=0.2)
    ap.add_argument("--p-out", type=float, default=0.02)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for dtype in (torch.float16, torch.float32):
        for name, A in (("arxiv-rmat", graphs.rmat_graph_n(169_343, 2_330_000, seed=5, device=dev, dtype=dtype)),
                        ("arxiv", graphs.uniform_graph(169_343, 2_330_000, seed=5, device=dev, dtype=dtype))):
            Wh = (torch.rand((A.n_rows, 256), generator=g, device=dev) - 0.5).to(dtype)
            att = ((torch.rand(512, generator=g, device=dev) - 0.5) / 8).to(dtype)
            leg(name, A, Wh, att)
        A = node_batch_hub(a.nodes, a.batch_size, a.p_in, a.p_out, dtype)
        Wh = (torch.rand((A.n_rows, a.hidden), generator=g, device=dev) - 0.5).to(dtype)
        att = ((torch.rand(2 * a.hidden, generator=g, device=dev) - 0.5) / 4).to(dtype)
        leg("node-batch-hub", A, Wh, att)


if __name__ == "__main__":
    main()
