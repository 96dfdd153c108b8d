#!/usr/bin/env python3
"""Digests of the small-graph stack (sgx_stack_forward, sgx_stack_backward, sgx_batch_plan_*, and one launch each of
sgx_gat_stack_forward and sgx_quant_stack_forward) for comparing two builds of the library bit for bit: one JSON line per
(element type, case) with the SHA-256 of the pooled output, of every D_l, dW_l and G_l, and of the plan's group table.
The cases are the CASES of tests/test_gpu_stack_train.py on that file's random_batch and seeds (one generator per case
gives the sizes, then the weights, then grad_pooled, as in the test), with six random graph sizes plus one of the backward
row budget, a 1-row and an empty graph; then an empty batch and the 20 000 small graphs of that file's
test_more_groups_than_the_grid: more groups than the backward's 512-wide grid (asserted), so that its workgroups take
several groups and all but the first add into the slice.
Before those, the Python above the library: train.StackTrainer (GCN and GAT model) and train.NodeTrainer (with a mask) on
the small fixtures of tests/test_gpu_trainer.py and tests/test_gpu_node_trainer.py, eager and replayed (trainer_lines),
and ops.GcnStack / GatStack / QuantStack through .apply and backward (autograd_lines).
Run it on each build and diff the outputs: a refactor of the stack's files, or of the Python that fills their
descriptors, changes no line."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sgracex1_amd import _lib, ops, quant  # noqa: E402
from test_gpu_stack_train import CASES, DEV, _budget, forward_outs, random_batch  # noqa: E402

NAMES = {torch.float16: "f16", torch.float32: "f32"}


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def weights_of(rng, widths):
    return [torch.tensor(rng.standard_normal((m, p)) / np.sqrt(m), device=DEV, dtype=torch.float32)
            for m, p in zip(widths[:-1], widths[1:])]


def empty_batch(dtype, m_in):
    i32 = dict(dtype=torch.int32, device=DEV)
    adj = ops.Csr(torch.zeros(1, **i32), torch.zeros(0, **i32), torch.zeros(0, dtype=dtype, device=DEV), 0)
    return adj, torch.zeros((0, m_in), dtype=dtype, device=DEV), torch.zeros(1, **i32)


def train_line(name, dtype, seed, rng, sizes, widths, relus, sparse, width, min_groups=0):
    """Forward and backward of one batch on a backward plan; rng: the generator that drew `sizes`."""
    adj, x, ptr = random_batch(seed, dtype, sizes, widths[0], sparse) if sizes else empty_batch(dtype, widths[0])
    weights = weights_of(rng, widths)
    plan = ops.BatchPlan.cached(adj, ptr, width, _lib.SGX_BATCH_BACKWARD)
    assert plan.fits and (not min_groups or plan.groups > min_groups), (name, plan.groups)
    pooled, outs = forward_outs(adj, x, weights, relus, ptr, plan)
    gp = torch.tensor(rng.standard_normal((len(sizes), widths[-1])), device=DEV, dtype=torch.float32)
    dW, G = ops.gcn_stack_backward(adj, x, weights, relus, ptr, outs, gp, plan=plan, want_G=True)
    torch.cuda.synchronize()
    rec = {"dtype": NAMES[dtype], "case": name, "rows": plan.rows, "groups": plan.groups, "group_graph": sha(plan.export_groups()),
           "pooled": sha(pooled)}
    for l in range(len(weights)):
        rec.update({f"D{l}": sha(outs[l]), f"dW{l}": sha(dW[l]), f"G{l}": sha(G[l])})
    return rec


def sizes_of(rng, R, n):
    sizes = [int(s) for s in rng.integers(1, R + 1, n)] + [R, 1, 0]
    sizes[0] = 5                                                     # graph 0: no edges
    sizes[3] = 0                                                     # an empty graph
    return sizes


def forms_lines(dtype):
    """One GAT-stack and one quantised-stack launch on case 0's shape: the group decode the three forward kernels share."""
    widths, relus, sparse = CASES[0]
    relus = [bool(r) for r in relus]
    rng = np.random.default_rng(4000 + (dtype == torch.float16))
    sizes = sizes_of(rng, _budget(dtype, max(widths[1:])), 6)
    adj, x, ptr = random_batch(4000, dtype, sizes, widths[0], sparse)
    adj = ops.Csr(adj.rowptr, adj.col, adj.val.abs(), adj.n_rows)     # (an edge is live where its value is positive)
    wts = [w.t().to(dtype).contiguous() for w in weights_of(rng, widths)]
    atts = [torch.tensor(rng.standard_normal(2 * p) * 0.3, device=DEV).to(dtype) for p in widths[1:]]
    plan = ops.BatchPlan.cached(adj, ptr, max(widths[1:]))
    pooled, outs = ops.gat_stack_forward(adj, x, wts, atts, relus, ptr, want_layer_outputs=True, plan=plan)
    yield dict({"dtype": NAMES[dtype], "case": "gat", "pooled": sha(pooled)}, **{f"D{l}": sha(o) for l, o in enumerate(outs)})
    if dtype != torch.float32:
        return
    qs = [quant.constants(8), quant.constants(8)]
    pooled, outs = ops.quant_stack_forward(adj, x, wts, [None, atts[1]], relus, ptr, qs, want_layer_outputs=True, plan=plan)
    yield dict({"dtype": NAMES[dtype], "case": "quant", "pooled": sha(pooled)}, **{f"D{l}": sha(o) for l, o in enumerate(outs)})


def autograd_lines(dtype):
    """ops.GcnStack, ops.GatStack and (float32: the quantised layers work on float32 buffers) ops.QuantStack through
    .apply and pooled.backward(gp) on CASES[0] and CASES[1]: the pooled output, every dW_l and every attention gradient.
    The quantised line of case 0 has a GCN layer 0 and the adjacency quantised beforehand, that of case 1 quantises it
    as it is read."""
    for case in (0, 1):
        widths, relus, sparse = CASES[case]
        relus = tuple(bool(r) for r in relus)
        n = len(relus)
        seed = 6000 + 10 * case + (dtype == torch.float16)
        width = max(widths[1:] + (() if sparse else widths[:1]))
        rng = np.random.default_rng(seed)
        sizes = sizes_of(rng, _budget(dtype, width), 6)
        adj, x, ptr = random_batch(seed, dtype, sizes, widths[0], sparse)
        adj = ops.Csr(adj.rowptr, adj.col, adj.val.abs(), adj.n_rows)     # (an edge is live where its value is positive)
        plan = ops.BatchPlan.cached(adj, ptr, width, _lib.SGX_BATCH_BACKWARD)
        assert plan.fits, (case, plan.rows)
        Ws = [w.requires_grad_(True) for w in weights_of(rng, widths)]
        atts = [torch.tensor(rng.standard_normal((2 * p, 1)) * 0.3, device=DEV, dtype=torch.float32).requires_grad_(True)
                for p in widths[1:]]
        gp = torch.tensor(rng.standard_normal((len(sizes), widths[-1])), device=DEV, dtype=torch.float32)
        qs = tuple(quant.constants(8) for _ in range(n))
        forms = [("GcnStack", Ws, lambda: ops.GcnStack.apply(adj, x, ptr, plan, relus, *Ws)),
                 ("GatStack", Ws + atts, lambda: ops.GatStack.apply(adj, x, ptr, plan, relus, 0.2, *Ws, *atts))]
        if dtype == torch.float32:
            q_atts = [None] + atts[1:] if case == 0 else atts
            adj_q = adj.quantized(qs[0]) if case == 0 else None
            forms.append(("QuantStack", Ws + [a for a in q_atts if a is not None],
                          lambda: ops.QuantStack.apply(adj, adj_q, x, ptr, plan, relus, 0.2, qs, *Ws, *q_atts)))
        for name, params, apply in forms:
            for p in params:
                p.grad = None
            pooled = apply()
            pooled.backward(gp)
            torch.cuda.synchronize()
            rec = {"dtype": NAMES[dtype], "case": f"{name}{case}", "pooled": sha(pooled.detach())}
            rec.update({f"dW{l}": sha(w.grad) for l, w in enumerate(Ws)})
            rec.update({f"dA{l}": sha(a.grad) for l, a in enumerate(atts) if any(a is p for p in params)})
            yield rec


def _mutag_models():
    """The models and the batch of tests/test_gpu_trainer.py: GCN_PYNQ (fp16) and GAT_POOL_PYNQ (fp32, attention) with
    train_stack on the 188 graphs of MUTAG."""
    import test_gpu_trainer as T
    from sgracex1_amd import config, sgrace
    b = T._mutag()
    yield "StackTrainer_gcn", T._gcn()[0], (b.x, b.edge_index, b.batch, b.y)
    saved = config.snapshot()
    config.acc, config.float_type, config.compute_attention = 1, np.float32, 1
    sgrace.init_SGRACE().register_map.layer_count = 2
    try:
        yield "StackTrainer_gat", T._gat(sgrace)[0], (b.x, b.edge_index, b.batch, b.y)
    finally:
        config.restore(saved)
        sgrace.init_SGRACE()


def _node_model():
    """The model, the 300-node graph and the mask of tests/test_gpu_node_trainer.py's `env`, with the attention aggregate."""
    import test_gpu_node_trainer as T
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, 1
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 1, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(7)
    x, ei, y = T._example().planted_partition(300, 5, 200, 0.05, 0.005, 3, torch.device(DEV))
    mask = torch.zeros(300, dtype=torch.bool, device=DEV)
    mask[torch.randperm(300, generator=torch.Generator().manual_seed(3)).to(DEV)[:60]] = True
    try:
        yield "NodeTrainer_mask", sgrace.GAT_PYNQ(200, 16, 1, 5).to(DEV).train(), (x, ei, y, mask)
    finally:
        config.restore(saved)
        sgrace.init_SGRACE()


def trainer_lines():
    """The three losses, and the parameters and both Adam moments after three eager steps and after three replays of a
    captured step from the same start (the parameters that receive a gradient: the others are never initialised)."""
    from sgracex1_amd import train
    for source, cls in ((_mutag_models, train.StackTrainer), (_node_model, train.NodeTrainer)):
        for name, model, batch in source():
            trainer = cls(model, lr=0.01, p_drop=0.5, seed=99)
            start = trainer.state()
            for leg in ("eager", "replay"):
                trainer.load_state(start)
                torch.manual_seed(5)
                step = (lambda: trainer.step(*batch)) if leg == "eager" else trainer.capture(*batch)
                losses = [step().clone() for _ in range(3)]
                torch.cuda.synchronize()
                n = len(trainer.params)
                live = [k for k, g in enumerate(trainer.last_grads) if g is not None]
                state = trainer.state()
                rec = {"case": name, "leg": leg, "t": int(state[-1].item()), "loss": [sha(v) for v in losses]}
                for tag, part in (("param", state[:n]), ("exp_avg", state[n:2 * n]), ("exp_avg_sq", state[2 * n:3 * n])):
                    rec[tag] = [sha(part[k]) for k in live]
                yield rec


def main():
    for rec in trainer_lines():
        print(json.dumps(rec), flush=True)
    for dtype in (torch.float16, torch.float32):
        for rec in autograd_lines(dtype):
            print(json.dumps(rec), flush=True)
        for case, (widths, relus, sparse) in enumerate(CASES):
            seed = 200 * case + (dtype == torch.float16)
            width = max(widths[1:] + (() if sparse else widths[:1]))
            rng = np.random.default_rng(seed)
            sizes = sizes_of(rng, _budget(dtype, width), 6)
            print(json.dumps(train_line(case, dtype, seed, rng, sizes, widths, [bool(r) for r in relus], sparse, width)), flush=True)
        for rec in forms_lines(dtype):
            print(json.dumps(rec), flush=True)
        widths, relus, sparse = CASES[0]
        relus = [bool(r) for r in relus]
        print(json.dumps(train_line("empty", dtype, 5000, np.random.default_rng(5000), [], widths, relus, False, 64)), flush=True)
        rng = np.random.default_rng(77)
        many = [int(s) for s in rng.integers(0, 24, 20000)]
        print(json.dumps(train_line("many", dtype, 78, rng, many, widths, relus, sparse, 64, min_groups=2 * 512)), flush=True)


if __name__ == "__main__":
    main()
