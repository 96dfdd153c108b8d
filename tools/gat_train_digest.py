#!/usr/bin/env python3
"""Digests of the GAT training path's kernels that share the long-row walk (long_rows.h) for comparing two builds of the
library bit for bit: one JSON line per (element type, graph, head layout) with the SHA-256 of every output of
ops.gat_aggregate(want_row_stats=True) (D and the four statistics arrays), ops.gat_edge_outputs and, with one head,
ops.gat_backward_edges, ops.gat_backward_edges_stats (with S_out) and ops.gat_attention_grad; on the square graph also
ops.layer_backward(gat=True) from E / S and from the statistics.  The graphs: tests/_gat_ref.adversarial_graph at the head
layouts of tests/test_gpu_gat_stats.py (rows of 256 and 257 entries, long rows with masked tasks, a dead long row) and the
power-law graph of tests/test_gpu_layer_backward.py (hub rows next to each other, rows without entries).  Run it on each
build (SGX_LIB_PATH names another build's library) and diff the outputs: a refactor of the walk changes no line."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gat_ref as R  # noqa: E402
from sgracex1_amd import ops  # noqa: E402

DTYPES = {"f16": torch.float16, "f32": torch.float32}
SHAPES = [(1, 64), (8, 32), (1, 256)]                    # heads x columns per head (tests/test_gpu_gat_stats.py)
dev = torch.device("cuda")


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(A, Wh, att, heads, seed, square):
    """Every entry point on adjacency A with the dead rows' mean fill; Wh, att of A's element type."""
    rec = {}
    dead_weight = 1.0 / A.n_cols
    D, stats = ops.gat_aggregate(A, Wh, att, alpha=0.2, heads=heads, fill_dead_rows=True, want_row_stats=True)
    rec["D"] = sha(D)
    for name, t in zip(("score_row", "score_col", "row_max", "row_sum"), stats.tensors()):
        rec[name] = sha(t)
    E, S = ops.gat_edge_outputs(A, stats, alpha=0.2, dead_weight=dead_weight)
    rec["E"], rec["S"] = sha(E), sha(S)
    if heads > 1:
        return rec
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    F = Wh.shape[1]
    G = torch.randn((A.n_rows, F), generator=gen, device=dev)
    Whf, dead = Wh.float().contiguous(), A.dead_rows
    sg, g1 = ops.gat_backward_edges(A, E, S, G, Whf, alpha=0.2, dead=dead)
    rec["bwd_sg"], rec["bwd_g1"] = sha(sg), sha(g1)
    sg2, g12, S_out = ops.gat_backward_edges_stats(A, stats, G, Whf, alpha=0.2, dead=dead, dead_weight=dead_weight)
    rec["bwd_stats_sg"], rec["bwd_stats_g1"], rec["bwd_stats_S_out"] = sha(sg2), sha(g12), sha(S_out)
    rec["attention_grad"] = sha(ops.gat_attention_grad(A, sg, g1, Whf))
    if square:
        M = 7
        X = torch.rand((A.n_rows, M), generator=gen, device=dev).half().float()
        W = (torch.rand((M, F), generator=gen, device=dev) - 0.5).half().float()
        for form, kw in (("es", dict(E=E, S=S)), ("stats", dict(stats=stats, dead_weight=dead_weight))):
            out = ops.layer_backward(A, X, W, G, gat=True, gemm_mode=1, alpha=0.2, dead=dead, **kw)
            for name, t in zip(("grad_input", "grad_weights", "grad_attention"), out):
                rec[f"layer_{form}_{name}"] = sha(t)
    return rec


def main():
    from test_gpu_layer_backward import _graph
    hub32 = _graph("rmat")
    for dt, tdt in DTYPES.items():
        for heads, f_head in SHAPES:
            g = R.adversarial_graph(dt, heads, f_head, seed=100 * heads + f_head)
            A = ops.Csr(torch.as_tensor(g["rowptr"], dtype=torch.int32, device=dev),
                        torch.as_tensor(g["col"], dtype=torch.int32, device=dev), torch.as_tensor(g["val"]).to(tdt).to(dev), g["n_cols"])
            Wh, att = torch.as_tensor(g["Wh"]).to(tdt).to(dev), torch.as_tensor(g["att"]).to(tdt).to(dev)
            rec = digests(A, Wh, att, heads, f_head, square=False)
            torch.cuda.synchronize()
            print(json.dumps(dict(dtype=dt, graph="adversarial", heads=heads, f_head=f_head, **rec)), flush=True)
        A = hub32.to(tdt)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(9)
        for F in (16, 64):
            Wh = (torch.randn((A.n_cols, F), generator=gen, device=dev) * 0.6).to(tdt)
            att = ((torch.rand(2 * F, generator=gen, device=dev) * 2 - 1) * 0.7).to(tdt)
            rec = digests(A, Wh, att, 1, F, square=True)
            torch.cuda.synchronize()
            print(json.dumps(dict(dtype=dt, graph="hub", heads=1, f_head=F, **rec)), flush=True)


if __name__ == "__main__":
    main()
