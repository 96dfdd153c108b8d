#!/usr/bin/env python3
"""What neighbour sampling costs (sgx_sample_neighbors, csrc/sample.hip): wall time per ops.sample_neighbors call,
stream synchronised, after warm-up, on the ogbn-products shape (2.45 M nodes, about 124 M edges; uniform and R-MAT),
batch 1024, fan-outs [15, 10, 5] and [10]; sampled edges per second; the same rule in plain torch ops on the same GPU
(the map-based relabel and Floyd's subset as tensor ops, its output checked equal); and one mini-batch training step
of examples/sgrace_node_classification.py (GCN and GAT).  One JSON line per measurement.

    python tools/sampler_probe.py > sampler.jsonl
    python tools/sampler_probe.py --quick          # only the kernels, for a rocprofv3 --kernel-trace --stats run
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgracex1_amd import graphs, ops  # noqa: E402

M32 = 0xFFFFFFFF


def _c(x):
    """uint64 constant as the int64 torch holds it."""
    return x - (1 << 64) if x >= 1 << 63 else x


def _shr(z, s):
    return (z >> s) & ((1 << (64 - s)) - 1)            # logical shift of an int64 tensor


def _mix64(z):
    z = (z ^ _shr(z, 30)) * _c(0xBF58476D1CE4E5B9)
    z = (z ^ _shr(z, 27)) * _c(0x94D049BB133111EB)
    return z ^ _shr(z, 31)


def _mix64_int(z):
    m = (1 << 64) - 1
    z &= m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def torch_sample(A, seeds, fanouts, seed=0, step=0):
    """The rule of include/sgx.h in torch ops: per hop, Floyd's subset as k vectorised steps over the rows that sample,
    positions sorted, first appearance by scatter_reduce(amin) into an n_nodes map, ids by cumsum.  -> n_id, rowptr,
    col, edge_pos."""
    dev = seeds.device
    rowptr, colidx = A.rowptr.long(), A.col.long()
    n_id = seeds.long()
    local = torch.full((A.n_rows,), -1, dtype=torch.int64, device=dev)
    local[n_id] = torch.arange(n_id.numel(), device=dev)
    f0, starts, cols, poss, e_total = 0, [], [], [], 0
    for h, k in enumerate(fanouts):
        key = _c(_mix64_int(_mix64_int(_mix64_int(seed) ^ step) ^ h))
        v = n_id[f0:]
        p0, deg = rowptr[v], rowptr[v + 1] - rowptr[v]
        cnt = deg if k < 0 else torch.clamp(deg, max=k)
        off = torch.cumsum(cnt, 0) - cnt
        starts.append(off + e_total)
        E = int(cnt.sum())
        row = torch.repeat_interleave(torch.arange(v.numel(), device=dev), cnt, output_size=E)
        rel = torch.arange(E, device=dev) - off[row]                 # position for take-all rows
        if k >= 0:
            big = torch.nonzero(deg > k).reshape(-1)
            if big.numel():
                d = deg[big]
                S = torch.full((big.numel(), k), -1, dtype=torch.int64, device=dev)
                for i in range(k):
                    j = d - k + i
                    r = _mix64(key ^ _mix64((v[big] << 32) | j))
                    m = j + 1
                    rh, rl = _shr(r, 32), r & M32
                    t = _shr(rh * m + _shr(rl * m, 32), 32)
                    hit = (S[:, :i] == t[:, None]).any(1)
                    S[:, i] = torch.where(hit, j, t)
                S = S.sort(1).values
                sel = torch.zeros(v.numel(), dtype=torch.bool, device=dev)
                sel[big] = True
                slot_of_row = torch.full((v.numel(),), -1, dtype=torch.int64, device=dev)
                slot_of_row[big] = torch.arange(big.numel(), device=dev)
                in_big = sel[row]
                rel[in_big] = S[slot_of_row[row[in_big]], rel[in_big]]
        pos = p0[row] + rel
        c = colidx[pos]
        ordinal = torch.arange(E, device=dev)
        first = torch.full((A.n_rows,), E, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, c, ordinal, "amin")
        new = (first[c] == ordinal) & (local[c] < 0)
        new_nodes = c[new]
        local[new_nodes] = n_id.numel() + torch.arange(new_nodes.numel(), device=dev)
        f0 = n_id.numel()
        n_id = torch.cat([n_id, new_nodes])
        cols.append(local[c])
        poss.append(pos)
        e_total += E
    rp = torch.full((n_id.numel() + 1,), e_total, dtype=torch.int64, device=dev)
    st = torch.cat(starts)
    rp[:st.numel()] = st
    return n_id, rp, torch.cat(cols), torch.cat(poss)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    shapes = [("products shape uniform", lambda: graphs.uniform_graph(2_450_000, 122_000_000, dtype=torch.float32,
                                                                      normalize=False)),
              ("products shape rmat", lambda: graphs.rmat_graph_n(2_450_000, 122_000_000, dtype=torch.float32,
                                                                  normalize=False))]
    for name, make in shapes:
        A = make()
        for fanouts in ([15, 10, 5], [10]):
            seeds = torch.randperm(A.n_rows, generator=torch.Generator().manual_seed(1))[:1024].to(dev)
            steps = iter(range(10 ** 9))
            ms, s = timed(lambda: ops.sample_neighbors(A, seeds, fanouts, seed=1, step=next(steps)), 5 if a.quick else 50)
            rec = {"graph": name, "nodes": A.n_rows, "nnz": A.nnz, "batch": 1024, "fanouts": fanouts,
                   "sample_ms": round(ms, 4), "sampled_nodes": s.n_id.numel(), "sampled_edges": s.adj.nnz,
                   "sampled_edges_per_s": round(s.adj.nnz / (ms * 1e-3), 1)}
            if not a.quick:
                tms, t = timed(lambda: torch_sample(A, seeds, fanouts, seed=1, step=7), 10)
                ref = ops.sample_neighbors(A, seeds, fanouts, seed=1, step=7)
                rec["torch_ops_ms"] = round(tms, 4)
                rec["torch_ops_equal"] = bool(torch.equal(t[0], ref.n_id.long()) and torch.equal(t[1], ref.adj.rowptr.long())
                                              and torch.equal(t[2], ref.adj.col[:ref.adj.nnz].long())
                                              and torch.equal(t[3], ref.edge_pos.long()))
                rec["speedup_vs_torch_ops"] = round(tms / ms, 2)
            print(json.dumps(rec), flush=True)
        del A
        torch.cuda.empty_cache()
    if a.quick:
        return
    # one mini-batch training step of the example (batch 128, [10, 10], 3000-node planted partition), after warm-up
    import importlib.util
    from sgracex1_amd import config, pyg_lite, sgrace
    spec = importlib.util.spec_from_file_location("nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, ei, y = mod.planted_partition(3000, 5, 200, 0.02, 0.002, 1, dev)
    train = torch.zeros(3000, dtype=torch.bool, device=dev)
    train[:600] = True
    for attention in (0, 1):
        config.acc, config.device, config.compute_attention = 1, "cuda", attention
        sgrace.init_SGRACE()
        model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        crit = torch.nn.CrossEntropyLoss()
        loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y, train_mask=train), [10, 10], batch_size=128,
                                         input_nodes=train, shuffle=True, seed=1)
        it = iter(loader)

        def step():
            nonlocal it
            try:
                b = next(it)
            except StopIteration:
                it = iter(loader)
                b = next(it)
            opt.zero_grad()
            out = model(b.x, b.edge_index.flip(0))
            loss = crit(out[b.train_mask], b.y[b.train_mask])
            loss.backward()
            opt.step()
            return b

        ms, b = timed(step, 50)
        print(json.dumps({"end_to_end": "example mini-batch training step (sample + gather + forward + backward + Adam)",
                          "model": "GAT" if attention else "GCN", "graph_nodes": 3000, "batch": 128, "fanouts": [10, 10],
                          "batch_nodes_last": b.num_nodes, "step_ms": round(ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
