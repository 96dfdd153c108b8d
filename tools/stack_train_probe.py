#!/usr/bin/env python3
"""What the fused training step (GCN_PYNQ(train_stack=True): sgx_stack_forward + sgx_stack_backward) saves against the
layer-by-layer training step (layer_count 1: FPYNQ / RPYNQ / ReadoutMean, one launch per stage each way).

Two workloads, MOL cell 18's model (7 -> 64 ReLU -> 64, mean pool, dropout, 64 -> 2 head, cross entropy), fp16 layers:
  mutag    the 188-graph MUTAG batch;
  big      MUTAG's graphs repeated to --graphs graphs (default 1,000,160: 5,320 copies, 17.9 M nodes, 39.6 M edges).
Per form: fwd_ms = the model's forward and the loss, step_ms = forward + loss + backward (no optimizer), bwd_ms = their
difference; hipEvents around --reps calls after warm-up, median of --trials.  graph_step_ms: the step replayed from a
hipGraph (null where the capture fails).  The two forms' losses are checked bit-equal first.  One JSON line each.

    python tools/stack_train_probe.py > stack_train.jsonl
    python tools/stack_train_probe.py --gat > profiles/r15_gat_stack_train.jsonl
        --gat = the SGRACE demo's graph classifier of attention layers instead (sgrace.GAT_POOL_PYNQ, fp32 layer buffers):
        GAT_POOL_PYNQ(train_stack=True) (sgx_gat_stack_forward + sgx_gat_stack_backward) against its layer-by-layer step,
        on the MUTAG batch only, eager and replayed.  The two forms' losses are not bit-equal there (the attention path's
        summation order is unpinned); the line records both.
    python tools/stack_train_probe.py --gat --quant 8 >> profiles/r16_quant_stack_train.jsonl
    python tools/stack_train_probe.py --quant 8 >> profiles/r16_quant_stack_train.jsonl
        --quant BITS = the same model under config.fake_quantization at BITS bits (with --gat attention layers, without it
        the library's GCN layers: config.compute_attention = 0): GAT_POOL_PYNQ(train_stack=True) (sgx_quant_stack_forward +
        sgx_quant_stack_backward) against its layer-by-layer quantised step.  --only big runs the repeated batch instead.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sgracex1_amd import _lib, molecule_gcn as M, ops, pynq_shim  # noqa: E402
from stack_probe import mutag_batch, time_ms  # noqa: E402


def model(form, dev):
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2 if form == "fused" else 1
    return M.GCN_PYNQ(64, 7, 2, ip, train_stack=form == "fused").to(dev).train()


def gat_main(args, dev):
    """The --gat lines: one per form on the MUTAG batch."""
    from sgracex1_amd import config, sgrace
    config.acc, config.compute_attention, config.float_type = 1, int(args.gat), np.float32
    if args.quant:
        config.fake_quantization, config.w_qbits = 1, args.quant
    ip = sgrace.init_SGRACE()
    big = args.only == "big"
    x, ei, batch, n_graphs = mutag_batch(max(1, args.graphs // 188) if big else 1, dev)
    reps = max(1, args.reps // 10) if big else args.reps
    y = torch.randint(0, 2, (n_graphs,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    crit = torch.nn.CrossEntropyLoss()
    torch.manual_seed(12345)
    models = {form: sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=form == "fused").to(dev).train() for form in ("fused", "chained")}
    models["chained"].load_state_dict(models["fused"].state_dict())

    def fwd(m):
        return crit(m(x, ei, batch), y)

    def step(m):
        m.zero_grad(set_to_none=True)
        loss = fwd(m)
        loss.backward()
        return loss

    for form, m in models.items():
        ip.register_map.layer_count = 2 if form == "fused" else 1
        torch.manual_seed(7)
        loss = float(step(m).detach())
        for _ in range(3):
            step(m)
        rec = {"workload": "big" if big else "mutag", "model": "gat" if args.gat else "gcn", "form": form, "graphs": n_graphs,
               "nodes": x.shape[0], "edges": ei.shape[1], "dtype": "f32", "first_loss": loss}
        if args.quant:
            rec["qbits"] = args.quant
        rec["fwd_ms"] = time_ms(lambda: fwd(m), reps, args.trials)
        rec["step_ms"] = time_ms(lambda: step(m), reps, args.trials)
        rec["bwd_ms"] = rec["step_ms"] - rec["fwd_ms"]
        rec["graph_step_ms"] = None
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    step(m)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            m.zero_grad(set_to_none=True)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fwd(m).backward()
            rec["graph_step_ms"] = time_ms(g.replay, reps, args.trials)
            del g
        except Exception as e:                          # (a path that synchronises cannot be captured)
            rec["graph_error"] = f"{type(e).__name__}: {str(e)[:120]}"
            torch.cuda.synchronize()
        rec["graphs_per_s_step"] = n_graphs / (rec["step_ms"] * 1e-3)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gat", action="store_true")
    ap.add_argument("--quant", type=int, default=0, choices=[0, 8, 4, 2, 1], metavar="BITS")
    ap.add_argument("--only", choices=["mutag", "big"], default=None)
    ap.add_argument("--graphs", type=int, default=1_000_160)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.gat or args.quant:
        return gat_main(args, dev)
    for name, copies in (("mutag", 1), ("big", max(1, args.graphs // 188))):
        if args.only and name != args.only:
            continue
        x, ei, batch, n_graphs = mutag_batch(copies, dev)
        y = torch.randint(0, 2, (n_graphs,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        crit = torch.nn.CrossEntropyLoss()
        models = {form: model(form, dev) for form in ("fused", "chained")}
        models["chained"].load_state_dict(models["fused"].state_dict())

        def fwd(m):
            return crit(m(1, x, ei, batch), y)

        def step(m):
            m.zero_grad(set_to_none=True)
            loss = fwd(m)
            loss.backward()
            return loss

        losses = {}
        for form, m in models.items():
            torch.manual_seed(7)
            losses[form] = step(m).detach()
        assert torch.equal(losses["chained"].view(torch.int32), losses["fused"].view(torch.int32)), "loss differs"
        adj = ops.cached_on(ei, ("adj_csr", x.shape[0], M.ACC_DTYPE),              # (the model's own, cached on ei)
                            lambda: ops.csr_from_edge_index(ei, x.shape[0], dtype=M.ACC_DTYPE))
        plan = ops.BatchPlan.cached(adj, ops.graph_ptr_of(batch), 64, _lib.SGX_BATCH_BACKWARD)
        reps = args.reps if name == "mutag" else max(1, args.reps // 10)
        for form, m in models.items():
            for _ in range(3):
                step(m)
            rec = {"workload": name, "form": form, "graphs": n_graphs, "nodes": x.shape[0], "edges": ei.shape[1],
                   "dtype": "f16", "bwd_plan_groups": plan.groups, "bwd_plan_rows": plan.rows}
            rec["fwd_ms"] = time_ms(lambda: fwd(m), reps, args.trials)
            rec["step_ms"] = time_ms(lambda: step(m), reps, args.trials)
            rec["bwd_ms"] = rec["step_ms"] - rec["fwd_ms"]
            rec["graph_step_ms"] = None
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        step(m)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                m.zero_grad(set_to_none=True)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    loss = fwd(m)
                    loss.backward()
                rec["graph_step_ms"] = time_ms(g.replay, reps, args.trials)
                del g
            except Exception as e:                          # (a path that synchronises cannot be captured)
                rec["graph_error"] = f"{type(e).__name__}: {str(e)[:120]}"
                torch.cuda.synchronize()
            rec["graphs_per_s_step"] = n_graphs / (rec["step_ms"] * 1e-3)
            print(json.dumps(rec), flush=True)
        del models


if __name__ == "__main__":
    main()
