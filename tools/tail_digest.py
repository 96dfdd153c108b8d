#!/usr/bin/env python3
"""Digests of the classifier tail (sgx_head_loss, sgx_node_loss, sgx_head_eval, sgx_node_eval, and the pooled means and
logits of sgx_readout_mean_linear) for comparing two builds of the library bit for bit: one JSON line per case with the
SHA-256 of every output buffer of each entry.  Run it on each build and diff the outputs: a refactor of the tail's files changes no line
(profiles/tail_digest_parent.jsonl and profiles/tail_digest.jsonl are such a pair).

The cases are the smallest shapes at which each path can still go wrong, on fixed seeds.  Node entries: n in 1, 15, 16, 17
and 16 * 512 + 5 (slice 0 walks a second block) at (P, C) = (1, 1), (7, 2), (64, 4), (64, 16), (256, 16) -- the kernel arms
of 1, 4, 16 and 64 accumulators -- and n = 17 at (1024, 16), past 64 KiB of LDS, with the toggles dealt round robin; then
at n = 17, (7, 2) every mask (none, all zero, about 30 %) with every n_prefix (0, 9, n), and every combination of the
bias, the logits output, the gradients and dropout (p = 0, p = 0.5, p = 0.5 with a device step); a target outside
0 .. C - 1 and a NaN in a selected row.  Head entries: G in 1, 3, 257 (a head_loss workgroup takes a second graph) and
1025 (a head_eval wave takes a second graph) at (P, C) = (1, 1), (7, 2), (64, 7), (1024, 64) with n_real in 0, 2, G and
the toggles dealt, then every combination of the toggles at G = 3.  A case is one line: node_loss's and node_eval's
buffers, or head_loss's (where n_real = G) and head_eval's.  The evaluation accumulators start non-zero in every other
case, and a second call into them is hashed too."""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgracex1_amd import ops  # noqa: E402

DEV = "cuda:0"
NODE_SHAPES = [(1, 1), (7, 2), (64, 4), (64, 16), (256, 16), (1024, 16)]
NODE_ROWS = [1, 15, 16, 17, 16 * 512 + 5]
HEAD_SHAPES = [(1, 1), (7, 2), (64, 7), (1024, 64)]
HEAD_GRAPHS = [1, 3, 257, 1025]
MASKS, PREFIXES, DROPS = ("none", "zero", "random"), (0, 9, "n"), ("p0", "p", "p_dev")


def sha(t):
    return None if t is None else hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def dev(a):
    return torch.as_tensor(a, device=DEV)


def operands(seed, n, P, C, bias):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, P)).astype(np.float32)
    W = (rng.standard_normal((C, P)) / np.sqrt(P)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32) if bias else None
    target = rng.integers(0, C, n).astype(np.int64)
    return rng, rows, W, b, target


def dropout_args(drop):
    """p, seed, step and the device step word of a DROPS entry."""
    step_dev = dev(np.array([3], np.int64)) if drop == "p_dev" else None
    return dict(p=0.0 if drop == "p0" else 0.5, seed=0x1234567890ABCDEF, step=41, step_dev=step_dev)


def accumulators(nonzero):
    return (dev(np.array([1000, 77] if nonzero else [0, 0], np.int64)), dev(np.array([12.625 if nonzero else 0.0], np.float64)))


def selection(rng, n, mask, prefix):
    m = None if mask == "none" else np.zeros(n, bool) if mask == "zero" else rng.random(n) < 0.3
    return (None if m is None else dev(m)), (n if prefix == "n" else prefix)


def node_lines(seed, n, P, C, mask, prefix, bias, logits, grads, drop, acc_nonzero, bad_target=False, nan=False, eval_too=True):
    rng, H, W, b, target = operands(seed, n, P, C, bias)
    if bad_target:
        target[0], target[n - 1] = C, -1
    if nan:
        H[min(3, n - 1), P // 2] = np.nan
    m, n_prefix = selection(rng, n, mask, prefix)
    H, W, b, target = dev(H), dev(W), None if b is None else dev(b), dev(target)
    case = dict(n=n, P=P, C=C, mask=mask, prefix=prefix, bias=bias, logits=logits, bad_target=bad_target, nan=nan)
    out = ops.node_loss(H, W, b, target, mask=m, n_prefix=n_prefix, grad_scale=1.5, want_logits=logits, want_counts=True,
                        grads=grads, **dropout_args(drop))
    names = ("loss", "grad_H", "grad_W", "grad_b", "counts", "logits")
    rec = dict(case, grads=grads, drop=drop, node_loss={k: sha(v) for k, v in zip(names, out)})
    if eval_too:
        rec["acc_nonzero"] = acc_nonzero
        totals, loss_sum = accumulators(acc_nonzero)
        for call in ("node_eval", "node_eval_again"):
            out = ops.node_eval(H, W, b, target, totals, loss_sum, mask=m, n_prefix=n_prefix, want_logits=logits)
            rec[call] = {k: sha(v) for k, v in zip(("totals", "loss_sum", "logits"), out)}
    yield rec


def head_lines(seed, G, P, C, n_real, bias, logits, drop, acc_nonzero, bad_target=False, eval_too=True):
    rng, pooled, W, b, target = operands(seed, G, P, C, bias)
    if bad_target:
        target[0], target[G - 1] = C, -1
    pooled, W, b, target = dev(pooled), dev(W), None if b is None else dev(b), dev(target)
    rec = dict(G=G, P=P, C=C, n_real=n_real, bias=bias, logits=logits, drop=drop, bad_target=bad_target)
    if n_real == G:                                                     # head_loss has no n_real
        out = ops.head_loss(pooled, W, b, target, grad_scale=1.5, want_logits=logits, **dropout_args(drop))
        names = ("loss", "grad_pooled", "grad_W", "grad_b", "logits")
        rec["head_loss"] = {k: sha(v) for k, v in zip(names, out)}
    if eval_too:
        rec["acc_nonzero"] = acc_nonzero
        totals, loss_sum = accumulators(acc_nonzero)
        for call in ("head_eval", "head_eval_again"):
            out = ops.head_eval(pooled, W, b, target, n_real=n_real, totals=totals, loss_sum=loss_sum, want_logits=logits)
            rec[call] = {k: sha(v) for k, v in zip(("totals", "loss_sum", "logits"), out)}
    yield rec


def readout_lines():
    for k, (dtype, (sizes, F, C)) in enumerate(itertools.product(
            (torch.float16, torch.float32), (([1], 1, 1), ([3, 0, 5, 1], 7, 2), ([9] * 5 + [40], 64, 7), ([2, 300, 1], 300, 64)))):
        bias = k % 2 == 0
        rng = np.random.default_rng(9000 + k)
        ptr = dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
        x = dev(rng.standard_normal((sum(sizes), F)).astype(np.float32)).to(dtype)
        W = dev((rng.standard_normal((C, F)) / np.sqrt(F)).astype(np.float32))
        b = dev(rng.standard_normal(C).astype(np.float32)) if bias else None
        logits, pooled = ops.readout_mean_linear(x, ptr, W, b, want_pooled=True)
        yield dict(entry="readout_mean_linear", dtype=str(dtype), sizes=sizes, F=F, C=C, bias=bias, pooled=sha(pooled),
                   logits=sha(logits))


def cases():
    seed = itertools.count(1)
    odd = lambda s: s % 2 == 1
    node_toggles = list(itertools.product(MASKS, PREFIXES, (True, False), (False, True), (True, False), DROPS))
    deal = itertools.cycle(node_toggles[::7])                            # 7 is coprime to every toggle's period
    for P, C in NODE_SHAPES[:-1]:
        for n in NODE_ROWS:
            s = next(seed)
            yield from node_lines(s, n, P, C, *next(deal), acc_nonzero=odd(s))
    for t in (("random", 9, True, True, True, "p_dev"), ("none", "n", False, False, False, "p0")):
        s = next(seed)
        yield from node_lines(s, 17, 1024, 16, *t, acc_nonzero=odd(s))
    for mask, prefix in itertools.product(MASKS, PREFIXES):              # the selection, at n = 17, (7, 2)
        s = next(seed)
        yield from node_lines(s, 17, 7, 2, mask, prefix, True, odd(s), True, "p", acc_nonzero=odd(s))
    for bias, logits, grads, drop in itertools.product((True, False), (False, True), (True, False), DROPS):
        s = next(seed)                                                   # (node_eval has neither of the last two toggles)
        yield from node_lines(s, 17, 7, 2, "random", 9, bias, logits, grads, drop, acc_nonzero=odd(s), eval_too=grads and drop == "p0")
    for extra in (dict(bad_target=True), dict(nan=True)):
        yield from node_lines(next(seed), 17, 64, 16, "none", "n", True, True, True, "p0", False, **extra)
    head_toggles = list(itertools.product((True, False), (False, True), DROPS))
    deal = itertools.cycle(head_toggles[::5])                            # 5 is coprime to 12
    for (P, C), G in itertools.product(HEAD_SHAPES, HEAD_GRAPHS):
        for n_real in sorted({0, min(2, G), G}):
            s = next(seed)
            yield from head_lines(s, G, P, C, n_real, *next(deal), acc_nonzero=odd(s))
    for t in head_toggles:                                               # every toggle, at G = 3, (7, 2)
        s = next(seed)
        yield from head_lines(s, 3, 7, 2, 3, *t, acc_nonzero=odd(s), eval_too=t[2] == "p0")
    yield from head_lines(next(seed), 3, 7, 2, 3, True, True, "p0", False, bad_target=True)
    yield from readout_lines()


if __name__ == "__main__":
    for rec in cases():
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
