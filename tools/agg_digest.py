#!/usr/bin/env python3
"""Digests of the plain aggregation on every kind of row schedule (the graphs of tests/test_gpu_row_schedule.py, whose degree
order ends in a tail of exactly 4096 one-step rows) for comparing two builds of the library bit for bit: one JSON line per
(element type, width, plan) with the SHA-256 of ops.spmm, of ops.spmm_acc's fp32 partial and of the pass that takes it in,
and of ops.xw_sparse on the same small matrix (under 2^20 entries: the gather kernel, not the LDS form).  Run it on each
build and diff the outputs: a refactor of the schedule changes no line."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _row_schedule_graphs as G  # noqa: E402
from sgracex1_amd import _lib, ops  # noqa: E402

DTYPES = {"f16": torch.float16, "f32": torch.float32}
WIDTHS = (64, 100, 32, 256)
# name: (tuning while the plan is built, or None for no plan; tuning while the kernels run)
PLANS = {
    "none": (None, {}),
    "tasks_natural": ({"SGX_PLAN_REORDER_BELOW": "0"}, {}),
    "tasks_ordered_tail": ({"SGX_PLAN_REORDER_BELOW": "2"}, {}),
    "tasks_ordered_no_short_tail": ({"SGX_PLAN_REORDER_BELOW": "2"}, {"SGX_SPMM_NO_SHORT_TAIL": "1"}),
}


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    dev = torch.device("cuda")
    for dt, tdt in DTYPES.items():
        g = G.graph("tail_4096", dt)
        rowptr, col = torch.as_tensor(g["rowptr"], device=dev), torch.as_tensor(g["col"], device=dev)
        val = torch.as_tensor(g["val"]).to(tdt).to(dev)
        for width in WIDTHS:
            H = torch.as_tensor(G.table(g["n"], width, seed=width)).to(tdt).to(dev)
            for name, (build, run) in PLANS.items():
                A = ops.Csr(rowptr, col, val, g["n"])
                if build is not None:
                    with _lib.tuning(**build):
                        A._plan = ops.Plan(rowptr)
                    assert A._plan.long_rows == 2 and A._plan.reordered == (name != "tasks_natural")
                use = build is not None
                with _lib.tuning(**run):
                    part = ops.spmm_acc(A, H, partial_out=True, use_plan=use)
                    rec = {"dtype": dt, "width": width, "plan": name, "spmm": sha(ops.spmm(A, H, relu=True, use_plan=use)),
                           "acc_partial": sha(part), "acc_final": sha(ops.spmm_acc(A, H, relu=True, acc_in=part, use_plan=use)),
                           "xw_sparse": sha(ops.xw_sparse(A, H, use_plan=use))}
                torch.cuda.synchronize()
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
