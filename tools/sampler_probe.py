#!/usr/bin/env python3
"""What neighbour sampling costs (sgx_sample_neighbors, csrc/sample.hip): wall time per ops.sample_neighbors call,
stream synchronised, after warm-up, on the ogbn-products shape (2.45 M nodes, about 124 M edges; uniform and R-MAT),
batch 1024, fan-outs [15, 10, 5] and [10]; sampled edges per second; the same rule in plain torch ops on the same GPU
(the map-based relabel and Floyd's subset as tensor ops, its output checked equal); and one mini-batch training step
of examples/sgrace_node_classification.py (GCN and GAT).  One JSON line per measurement.

    python tools/sampler_probe.py > sampler.jsonl
    python tools/sampler_probe.py --quick          # only the kernels, for a rocprofv3 --kernel-trace --stats run
    python tools/sampler_probe.py --node-batch [--arms default] [--trace]
    python tools/sampler_probe.py --node-batch --replay replay|eager [--label L]    # profiles/r22_node_replay.jsonl
    python tools/sampler_probe.py --node-batch --replay replay|eager --quant 8      # profiles/r24_node_replay_quant.jsonl
                                                   # the training step through the default and the prepared NeighborLoader
                                                   # (GCN and GAT, the example's shape and the ogbn-products shape), the arms
                                                   # interleaved, median of repeated windows and their spread; and the batch
                                                   # preparation alone, device launches against the torch ops
                                                   # (profiles/r08_node_batch.jsonl).  --arms default: on a tree without
                                                   # the prepared loader.  --trace: few steps, for rocprofv3 --kernel-trace
                                                   # --accb 0,1: config.accb of the step (the layer backward composed /
                                                   # as one call), every (arm, accb) pair a leg of the same windows
                                                   # (profiles/r09_layer_backward.jsonl); --label NAME tags the run
                                                   # --transposed: beside the prepared arm a "prepared_t" arm, the same
                                                   # loader with transposed=True (X^T and the GAT backward's transposed
                                                   # pattern built behind the sampler), in the same windows
                                                   # (profiles/r11_step_*.jsonl)
                                                   # --quant QBITS: the QUANTISED model (config.fake_quantization and
                                                   # hardware_quantize, w_qbits = QBITS), GCN, GAT and lean GAT, through
                                                   # the prepared loader without quant= (arm "prepared") and with it (arm
                                                   # "prepared_q", beside --arms), and the preparation alone of both
                                                   # (profiles/r12_node_batch_quant.jsonl; --arms prepared runs on a tree
                                                   # without quant=)
    python tools/sampler_probe.py --wide [--label L]    # profiles/sampler_wide.jsonl: ops.sample_neighbors alone at fan-outs
                                                   # over 64 -- [100], [256], [1024], [100, 10] -- beside the controls [10]
                                                   # and [15, 10, 5] and the one-lane path at [1025] (batch 16), both
                                                   # products shapes, batch 1024; then the node example's replayed step at
                                                   # [100, 10], unquantised.  One process = one run of every leg; run two
                                                   # checkouts alternately, three processes each, and hold a leg against
                                                   # the other checkout's run-to-run spread
    python tools/sampler_probe.py --wide-summary FILE   # those run lines and a summary line per leg
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


def node_batch(arms, trace, accbs=(0,), qbits=None):
    """The training step (loader, forward, loss, backward, Adam) per loader, and the preparation alone."""
    import importlib.util
    import statistics
    from sgracex1_amd import config, pyg_lite, quant, sgrace
    dev = torch.device("cuda")
    spec = importlib.util.spec_from_file_location("nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def example_shape():
        x, ei, y = mod.planted_partition(3000, 5, 200, 0.02, 0.002, 1, dev)
        train = torch.zeros(3000, dtype=torch.bool, device=dev)
        train[:600] = True
        return "example (3 000 nodes)", x, ei, y, train, 128, [10, 10]

    def products_shape():
        n, f = 2_450_000, 100
        A = graphs.uniform_graph(n, 122_000_000, dtype=torch.float32, normalize=False)
        row = torch.repeat_interleave(torch.arange(n, device=dev), (A.rowptr[1:] - A.rowptr[:-1]).long(), output_size=A.nnz)
        ei = torch.stack([A.col[:A.nnz].long(), row])           # CSR row = target of the edge
        del A, row
        g = torch.Generator(device=dev).manual_seed(1)
        x = (torch.rand((n, f), device=dev, generator=g) < 0.1).float() * torch.rand((n, f), device=dev, generator=g)
        y = torch.randint(0, 5, (n,), device=dev, generator=g)
        train = torch.zeros(n, dtype=torch.bool, device=dev)
        train[torch.randperm(n, device=dev, generator=g)[:200_000]] = True
        return "products shape uniform", x, ei, y, train, 1024, [15, 10, 5]

    for make in (example_shape, products_shape):
        name, x, ei, y, train, bs, fan = make()
        data = pyg_lite.NodeData(x, ei, y, train_mask=train)
        loaders = {}
        for arm in arms:
            kw = {"prepare": "sym_norm2"} if arm.startswith("prepared") else {}
            if arm == "prepared_t":
                kw["transposed"] = True
            if arm == "prepared_q":
                kw["quant"] = quant.constants(qbits)
            loaders[arm] = pyg_lite.NeighborLoader(data, fan, batch_size=bs, input_nodes=train, shuffle=True, seed=1, **kw)
        del ei
        for attention, lean in ((0, False), (1, False)) + (((1, True),) if qbits else ()):
            config.acc, config.device, config.compute_attention = 1, "cuda", attention
            config.gat_edge_outputs = 0 if lean else 1
            if qbits:
                config.fake_quantization = config.hardware_quantize = 1
                config.w_qbits = qbits
            sgrace.init_SGRACE()
            steps = {}
            # a leg = (loader arm, config.accb): every leg has its own model and takes its turn in every window
            legs = [(arm, accb) for arm in arms for accb in accbs]
            for arm, accb in legs:
                torch.manual_seed(0)
                model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(dev)
                opt = torch.optim.Adam(model.parameters(), lr=0.01)
                crit = torch.nn.CrossEntropyLoss()
                state = {"it": iter(loaders[arm])}

                def step(arm=arm, model=model, opt=opt, crit=crit, state=state, accb=accb):
                    config.accb = accb                          # read by the layers' forward, which fixes the backward's path
                    try:
                        b = next(state["it"])
                    except StopIteration:
                        state["it"] = iter(loaders[arm])
                        b = next(state["it"])
                    opt.zero_grad()
                    if arm.startswith("prepared"):
                        out = model(b.x, b.edge_index_agg)
                        loss = crit(out[:b.batch_size], b.y[:b.batch_size])
                    else:
                        out = model(b.x, b.edge_index.flip(0))
                        loss = crit(out[b.train_mask], b.y[b.train_mask])
                    loss.backward()
                    opt.step()
                    return b
                steps[(arm, accb)] = step
            windows, reps = (1, 3) if trace else (7, 30)
            times = {leg: [] for leg in legs}
            for leg in legs:                                    # warm-up of every leg before any timed window
                for _ in range(5):
                    b = steps[leg]()
            torch.cuda.synchronize()
            for _ in range(windows):                            # the legs interleaved, window by window
                for leg in legs:
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        b = steps[leg]()
                    torch.cuda.synchronize()
                    times[leg].append((time.perf_counter() - t0) / reps * 1e3)
            config.accb = 0
            for arm, accb in legs:
                v = times[(arm, accb)]
                print(json.dumps({"end_to_end": "mini-batch training step (loader + forward + loss + backward + Adam)",
                                  "loader": arm, "accb": accb, "model": ("GAT lean" if lean else "GAT") if attention else "GCN",
                                  **({"w_qbits": qbits} if qbits else {}), "graph": name, "batch": bs,
                                  "fanouts": fan, "batch_nodes_last": b.num_nodes, "step_ms_median": round(statistics.median(v), 4),
                                  "step_ms_min": round(min(v), 4), "step_ms_max": round(max(v), 4), "windows": windows,
                                  "steps_per_window": reps}), flush=True)
        config.gat_edge_outputs = 1
        if qbits and not trace:
            # the batch preparation alone, on the same seeds, with and without the quantised adjacency
            count = iter(range(10 ** 9))
            for arm in arms:
                if arm.startswith("prepared"):
                    ld = loaders[arm]
                    ms, _ = timed(lambda: ld._prepared(ld.input_nodes[:bs], None, next(count)), 50)
                    print(json.dumps({"batch_preparation": "NeighborLoader._prepared, stream synchronised", "loader": arm,
                                      "w_qbits": qbits, "graph": name, "batch": bs, "fanouts": fan, "ms": round(ms, 4)}), flush=True)
        elif "prepared" in arms and not trace:
            # the batch preparation alone, on the same seeds: one device call against the sampler plus today's torch ops
            ld = loaders["prepared"]
            seeds = ld.input_nodes[:bs]
            count = iter(range(10 ** 9))

            def device_form():
                return ld._prepared(seeds, None, next(count))

            def torch_form():
                s = ops.sample_neighbors(ld.csr, seeds, fan, seed=1, step=next(count))
                A = s.adj
                n_idx = s.n_id.long()
                target = torch.repeat_interleave(torch.arange(A.n_rows, device=dev), (A.rowptr[1:] - A.rowptr[:-1]).long(),
                                                 output_size=A.nnz)
                bx = ops.pack_rows(x, s.n_id)
                agg = torch.stack([A.col[:A.nnz].long(), target]).flip(0)
                e2, norm = sgrace.sym_norm2(agg, A.n_rows)
                adj = sgrace._edge_csr(None, e2, norm, A.n_rows, torch.float32)
                fea = ops.Csr.from_dense(bx, torch.float32)
                return adj.has_dead_rows, fea, y[n_idx], train[n_idx]

            a_ms, _ = timed(device_form, 50)
            b_ms, _ = timed(torch_form, 50)
            print(json.dumps({"batch_preparation": "sample + normalised CSR + feature CSR + x, y, mask + dead rows", "graph": name,
                              "batch": bs, "fanouts": fan, "device_launches_ms": round(a_ms, 4), "torch_ops_ms": round(b_ms, 4),
                              "speedup": round(b_ms / a_ms, 2)}), flush=True)
        del data, loaders, x, y, train
        torch.cuda.empty_cache()


def node_replay(leg, qbits=None):
    """--node-batch --replay: the NodeTrainer mini-batch step on the example's graph at batch 128 and [10, 10], GCN and
    attention, as ONE leg per process so that two checkouts can take turns in one visit: leg "replay" -- the padded loader
    and NodeTrainer.capture_loader's recorded step; leg "eager" -- NodeTrainer.step on the prepared loader's batches (runs
    on a checkout without padded batches too).  640 training nodes: five full batches an epoch, no short one.
    qbits (--quant): the QUANTISED model (config.fake_quantization and hardware_quantize) from loaders with quant= -- the
    eager leg runs on a checkout without padded quantised batches too (profiles/r24_node_replay_quant.jsonl) -- and the
    evaluation pass over the same loader: NodeTrainer.capture_eval_loader against evaluate(into=) per batch."""
    import importlib.util
    import statistics
    from sgracex1_amd import config, pyg_lite, quant, sgrace
    from sgracex1_amd.train import EvalSums
    from sgracex1_amd.train import NodeTrainer
    dev = torch.device("cuda")
    spec = importlib.util.spec_from_file_location("nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, ei, y = mod.planted_partition(3000, 5, 200, 0.02, 0.002, 1, dev)
    train = torch.zeros(3000, dtype=torch.bool, device=dev)
    train[:640] = True
    data = pyg_lite.NodeData(x, ei, y, train_mask=train)
    bs, fan, windows, epochs = 128, [10, 10], 7, 6
    for attention in (0, 1):
        config.acc, config.accb, config.device, config.compute_attention, config.gat_edge_outputs = 1, 0, "cuda", attention, 1
        if qbits:
            config.fake_quantization = config.hardware_quantize = 1
            config.w_qbits = qbits
        sgrace.init_SGRACE()
        torch.manual_seed(0)
        model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(dev).train()
        trainer = NodeTrainer(model, lr=0.01)
        kw = dict(batch_size=bs, input_nodes=train, shuffle=True, seed=1, prepare="sym_norm2", transposed=bool(attention))
        if qbits:
            kw["quant"] = quant.constants(qbits)
        extra = {}
        if leg == "replay":
            loader = pyg_lite.NeighborLoader(data, fan, pad=True, **kw)
            epoch = trainer.capture_loader(loader)
            live = torch.zeros(4, dtype=torch.int64, device=dev)

            def one_epoch():
                return epoch()
        else:
            loader = pyg_lite.NeighborLoader(data, fan, **kw)

            def one_epoch():
                return [trainer.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size) for b in loader]

        def windows_of(run):
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            out = []
            for _ in range(windows):
                t0 = time.perf_counter()
                for _ in range(epochs):
                    k = run()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) / (epochs * k) * 1e3)
            return out, k

        times, n_steps = windows_of(lambda: len(one_epoch()))
        if qbits:
            # the evaluation pass over the same loader and model: one recorded evaluation per full batch against
            # evaluate(into=) per batch; timed per batch of the pass
            if leg == "replay":
                run_pass = trainer.capture_eval_loader(loader)
            else:
                sums = EvalSums(dev)

                def run_pass():
                    sums.zero_()
                    for b in loader:
                        trainer.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size, into=sums)
                    return sums
            ev, _ = windows_of(lambda: (run_pass(), len(loader))[1])
            extra_eval = {"qbits": qbits, "eval_batch_ms_median": round(statistics.median(ev), 4), "eval_batch_ms_min": round(min(ev), 4),
                          "eval_batch_ms_max": round(max(ev), 4)}
        else:
            extra_eval = {}
        if leg == "replay":
            loader.status()
            seen = 0
            for seeds, _, step in loader.epoch_batches():          # the live counts of one more epoch, summed on the device
                loader.load(seeds, step)
                epoch.replay()
                live += loader.counts[:4]
                seen += 1
            cap = loader.capacity
            mean = [round(v / seen, 1) for v in live.tolist()]
            extra = {"padded_rows": cap.n_rows, "padded_adj_entries": cap.nnz_norm, "padded_fea_entries": cap.nnz_fea,
                     "padded_edges": cap.n_edges, "live_rows_mean": mean[0], "live_edges_mean": mean[1],
                     "live_adj_entries_mean": mean[2], "live_fea_entries_mean": mean[3]}
        print(json.dumps({"end_to_end": "NodeTrainer mini-batch step (sample + preparation + layers + loss + backward + Adam)",
                          "leg": leg, "model": "GAT" if attention else "GCN", "graph": "example (3 000 nodes)", "batch": bs,
                          "fanouts": fan, "steps_per_epoch": n_steps, "step_ms_median": round(statistics.median(times), 4),
                          "step_ms_min": round(min(times), 4), "step_ms_max": round(max(times), 4), "windows": windows,
                          "steps_per_window": epochs * n_steps, **extra_eval, **extra}), flush=True)


WIDE_LEGS = (([100], 1024), ([256], 1024), ([1024], 1024), ([100, 10], 1024), ([10], 1024), ([15, 10, 5], 1024), ([1025], 16))


def wide(label):
    """--wide: ops.sample_neighbors alone, stream synchronised, per leg three warm-up calls and five windows (every call a
    new step, so a new draw); the sampled edges of the last call and the share of its frontier rows whose degree exceeds
    their hop's fan-out (the rows that run the subset step).  ops.sample_form, where the checkout has it, names the form."""
    import statistics
    dev = torch.device("cuda")
    form = getattr(ops, "sample_form", None)
    shapes = [("products shape uniform", lambda: graphs.uniform_graph(2_450_000, 122_000_000, dtype=torch.float32,
                                                                      normalize=False)),
              ("products shape rmat", lambda: graphs.rmat_graph_n(2_450_000, 122_000_000, dtype=torch.float32,
                                                                  normalize=False))]
    for name, make in shapes:
        A = make()
        deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
        for fanouts, batch in WIDE_LEGS:
            seeds = torch.randperm(A.n_rows, generator=torch.Generator().manual_seed(1))[:batch].to(dev)
            steps = iter(range(10 ** 9))
            call = lambda: ops.sample_neighbors(A, seeds, fanouts, seed=1, step=next(steps))
            call()                                                   # warm-up: code objects, the workspace, the map
            torch.cuda.synchronize()

            def window(reps):
                t0 = time.perf_counter()
                for _ in range(reps):
                    out = call()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / reps * 1e3, out
            ms1, _ = window(1)
            reps = max(1, min(50, int(200 / max(ms1, 1e-3))))        # windows of about 0.2 s, 50 calls at the most
            runs = [window(reps) for _ in range(5)]
            windows, s = sorted(r[0] for r in runs), runs[-1][1]
            rows = over = 0
            for h, k in enumerate(fanouts):
                d = deg[s.n_id[(s.hop_nodes[h - 1] if h else 0):s.hop_nodes[h]].long()]
                rows, over = rows + d.numel(), over + int((d > k).sum())
            print(json.dumps({"label": label, "leg": "sample_neighbors", "graph": name, "batch": batch, "fanouts": fanouts,
                              "forms": [form(k) for k in fanouts] if form else None,
                              "ms_per_call": [round(v, 4) for v in windows], "ms_median": round(statistics.median(windows), 4),
                              "calls_per_window": reps, "sampled_edges": s.adj.nnz, "sampled_nodes": s.n_id.numel(),
                              "frontier_rows": rows, "share_of_rows_over_fanout": round(over / max(rows, 1), 4)}), flush=True)
        del A, deg
        torch.cuda.empty_cache()
    wide_step(label)


def wide_step(label):
    """The node example's replayed training step at batch 128 and fan-outs [100, 10] in the configuration of
    tools/quant_flat_probe.py's leg a, unquantised: NeighborLoader(pad=True, schedule="flat") through
    NodeTrainer.capture_loader, ms per step of a replayed epoch of ten steps, five epochs."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from sgrace_node_classification import planted_partition
    from sgracex1_amd import config, pyg_lite, sgrace
    from sgracex1_amd.train import NodeTrainer
    for attention in (0, 1):
        config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, attention
        config.fake_quantization = config.hardware_quantize = 0
        config.w_qbits, config.gat_edge_outputs, config.device = 32, 0, "cuda"
        sgrace.init_SGRACE()
        torch.manual_seed(1)
        n = 3000
        x, edge_index, y = planted_partition(n, 5, 200, 0.2, 0.02, 1, torch.device("cuda"))
        train = torch.zeros(n, dtype=torch.bool, device="cuda")
        train[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:1280].cuda()] = True      # ten full batches
        data = pyg_lite.NodeData(x, edge_index, y, train_mask=train)
        model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).cuda().train()
        trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=1)
        loader = pyg_lite.NeighborLoader(data, [100, 10], pad=True, schedule="flat", batch_size=128, input_nodes=train,
                                         shuffle=True, seed=1, prepare="sym_norm2", fill=1, transposed=True)
        epoch = trainer.capture_loader(loader)
        epoch()
        ms = sorted(timed(epoch, 1)[0] / len(loader) for _ in range(5))
        loader.status()
        print(json.dumps({"label": label, "leg": "replayed step", "route": "flat-replayed", "attention": bool(attention),
                          "graph": "example (3 000 nodes)", "batch": 128, "fanouts": [100, 10],
                          "ms_per_step": [round(v, 4) for v in ms], "steps_per_epoch": len(loader)}), flush=True)


def wide_summary(path):
    """--wide-summary FILE: the run lines of FILE (labels "parent" and "this", --wide's output of several processes) and,
    per leg, a summary line: the run medians of both, the parent's run-to-run spread of medians, the gap from this
    commit's worst median to the parent's best, and the verdict -- a win only where the gap exceeds that spread and every
    window of this commit lies below every window of the parent; "inside the spread" where the medians of this commit lie
    within the parent's range widened by its spread; "not measured" where a label has fewer than two runs."""
    import statistics
    runs, order = {}, []
    for line in open(path):
        rec = json.loads(line)
        print(json.dumps(rec))
        if "leg" not in rec or rec.get("label") not in ("parent", "this"):
            continue
        key = (rec["leg"], rec["graph"], rec.get("attention"), tuple(rec["fanouts"]), rec["batch"])
        if key not in runs:
            order.append(key)
        runs.setdefault(key, {"parent": [], "this": []})[rec["label"]].append(rec.get("ms_per_call") or rec["ms_per_step"])
    for key in order:
        what = {"summary_of": key[0], "graph": key[1], "fanouts": list(key[3]), "batch": key[4],
                **({} if key[2] is None else {"attention": key[2]})}
        r = runs[key]
        if min(len(r["parent"]), len(r["this"])) < 2:
            print(json.dumps(dict(what, status="not measured", runs={k: len(v) for k, v in r.items()})))
            continue
        med = {k: [statistics.median(v) for v in r[k]] for k in r}
        spread = max(med["parent"]) - min(med["parent"])
        gap = min(med["parent"]) - max(med["this"])
        below = max(max(v) for v in r["this"]) < min(min(v) for v in r["parent"])
        inside = min(med["parent"]) - spread <= min(med["this"]) and max(med["this"]) <= max(med["parent"]) + spread
        print(json.dumps(dict(what, unit="ms", parent_run_medians=med["parent"], this_run_medians=med["this"],
                              parent_run_to_run_spread_of_medians=round(spread, 4),
                              gap_parent_best_median_minus_this_worst_median=round(gap, 4),
                              verdict="win" if gap > spread and below else "inside the spread" if inside else "no claim")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--node-batch", action="store_true")
    ap.add_argument("--accb", default="0", help="--node-batch: config.accb of the training steps, a comma list (0,1 times "
                                                "both settings in the same interleaved windows)")
    ap.add_argument("--label", default=None, help="--node-batch: a tag printed with the run (which checkout this is)")
    ap.add_argument("--arms", default="default,prepared")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--quant", type=int, default=None, choices=[8, 4, 2, 1],
                    help="--node-batch: the quantised model at this w_qbits; adds the arm prepared_q where --arms holds prepared_q "
                         "or is left at its default")
    ap.add_argument("--transposed", action="store_true", help="--node-batch: add the arm prepared_t (the prepared loader with "
                                                              "transposed=True) to the same windows")
    ap.add_argument("--replay", default=None, choices=["replay", "eager"],
                    help="--node-batch: one leg of the replayed-step measurement (profiles/r22_node_replay.jsonl): 'replay' = "
                         "the padded loader through NodeTrainer.capture_loader, 'eager' = NodeTrainer.step on the prepared "
                         "loader (also on a checkout without padded batches); run the two alternately, a process each")
    ap.add_argument("--wide", action="store_true", help="fan-outs over 64: one run of every leg of profiles/sampler_wide.jsonl "
                                                        "(--label names the checkout)")
    ap.add_argument("--wide-summary", default=None, metavar="FILE", help="the run lines of FILE followed by one summary line "
                                                                         "per leg (needs no device)")
    a = ap.parse_args()
    if a.wide_summary:
        return wide_summary(a.wide_summary)
    if a.wide:
        return wide(a.label)
    if a.node_batch:
        if a.label:
            print(json.dumps({"label": a.label}), flush=True)
        if a.replay:
            return node_replay(a.replay, a.quant)
        arms = a.arms.split(",") + (["prepared_t"] if a.transposed else [])
        if a.quant and a.arms == "default,prepared":
            arms = ["prepared", "prepared_q"] + arms[2:]
        return node_batch(arms, a.trace, tuple(int(b) for b in a.accb.split(",")), a.quant)
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
