#!/usr/bin/env python3
"""Digests of every form of the GAT aggregate (the FORMS of tests/test_gpu_gat_paths.py, on that test's adversarial
graphs) for comparing two builds of the library bit for bit: one JSON line per (element type, head layout, form) with
the SHA-256 of D, of E and S where the form returns them, and the scratch size sgx_gat_scratch_bytes states for the call.
Run it on each build and diff the outputs: a refactor of the kernels' files or of the scratch layout changes no line."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sgracex1_amd import _lib  # noqa: E402
from test_gpu_gat_paths import FORMS, Case  # noqa: E402

LAYOUTS = [(1, 64), (1, 256), (3, 50), (4, 32), (66, 2)]


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    for dt in ("f16", "f32"):
        for heads, f_head in LAYOUTS:
            c = Case(dt, heads, f_head)
            for form, (tune, plan_kind, entry, want_es, rule) in FORMS.items():
                A = c.csr(plan_kind)
                plan = A._gat_plan.handle if plan_kind is not None else None
                with _lib.tuning(**tune):
                    got = c.run(A, entry, want_es, rule, rule != "zero")
                    scratch = _lib.lib.sgx_gat_scratch_bytes(c.g["n_cols"], heads * f_head, heads, int(rule == "mean"), plan)
                torch.cuda.synchronize()
                rec = {"dtype": dt, "heads": heads, "f_head": f_head, "form": form, "scratch_bytes": int(scratch)}
                rec.update({k: sha(v) for k, v in got.items()})
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
