"""Restatement of the evaluation head's rule (include/sgx.h, "the evaluation head") in numpy: the logits in the kernel's
stated fp32 order (correctly rounded fmaf chains per lane, the xor butterfly, the bias), a float64 reference of the
per-row cross entropy with the bound of the fp32 kernel's summed loss derived from its operation counts, the arg-max with
the first maximum winning, and the inputs the tests run.

u, gamma and the per-row bound are _train_tail_ref's (the per-row term is sgx_head_loss's).  Nothing here is tuned to
what the kernel returns."""
import numpy as np

from _train_tail_ref import K_EXP, K_LOG, U, gamma, head_f64

U64 = 2.0 ** -53                                   # float64's unit roundoff: the row losses are added in double
TINY = float(np.finfo(np.float32).tiny)

GRAPHS = [1, 2, 63, 64, 65, 257]                   # one row, the wavefront's edges, past sgx_head_loss's 256 slices
WIDTHS = [1, 64, 65]
CLASSES = [1, 2, 7]


def n_reals(G):
    return sorted({0, 1, G - 1, G})


def fmaf(a, b, c):
    """fl32(a * b + c) with one rounding, on float32 arrays.  The product of two float32 is exact in float64; the sum is
    formed in float64 with its rounding error (TwoSum) and rounded to odd, which makes the final rounding to float32 the
    correct one (53 >= 2 * 24 + 2)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bp = s - p
    err = (p - (s - bp)) + (c - bp)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def logits_f32(pooled, W, bias):
    """z [G, C] float32 in the rule's order: lane l an fmaf chain from 0 over j = l, l + 64, ...; the lanes added by the
    xor butterfly 32, 16, .. 1; then + bias[c]."""
    pooled, W = np.asarray(pooled, np.float32), np.asarray(W, np.float32)
    (G, P), C = pooled.shape, W.shape[0]
    lanes = np.zeros((G, C, 64), np.float32)
    for j0 in range(0, P, 64):
        n = min(64, P - j0)
        lanes[:, :, :n] = fmaf(np.broadcast_to(W[None, :, j0:j0 + n], (G, C, n)),
                               np.broadcast_to(pooled[:, None, j0:j0 + n], (G, C, n)), lanes[:, :, :n])
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, :, idx ^ off]).astype(np.float32)
    z = lanes[:, :, 0]
    return z if bias is None else (z + np.asarray(bias, np.float32)[None, :]).astype(np.float32)


def argmax_first(z):
    """The rule's arg-max per row: c ascending with a strict > from z[0], a NaN z[0] counting as -inf."""
    best = np.zeros(z.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        bv = np.where(z[:, 0] == z[:, 0], z[:, 0], -np.inf)
        for c in range(1, z.shape[1]):
            better = z[:, c] > bv
            bv, best = np.where(better, z[:, c], bv), np.where(better, c, best)
    return best


def eval_ref(pooled, W, bias, target, n_real):
    """(totals = (n_real, hits), loss_sum in float64, the bound of the kernel's loss_sum against it) of the first n_real
    rows.  hits come from the fp32 logits, as the kernel's do.

    The bound: per row _train_tail_ref.head_bounds' e_loss_g (the logits' gamma(P + 1) bound carried through lse and the
    subtraction); the rows' fp32 losses are then added in double, n_real additions from 0.0 and one more into the
    accumulator: gamma64(n_real + 1) times the sum of their magnitudes.  With C == 1 the kernel's loss is an exact 0
    (lse == z) and so is float64's."""
    pooled, W = np.asarray(pooled, np.float32)[:n_real], np.asarray(W, np.float32)
    t = np.asarray(target, np.int64)[:n_real]
    C = W.shape[0]
    if n_real == 0:
        return (0, 0), 0.0, 0.0
    live = (t >= 0) & (t < C)
    z32 = logits_f32(pooled, W, bias)
    hits = int((live & (argmax_first(z32) == t)).sum())
    _, z, _, _, _, aux = head_f64(pooled, W, bias, t)
    x, lse, onehot, b = aux["x"], aux["lse"], aux["onehot"], aux["b"]
    P = x.shape[1]
    if C == 1:
        return (n_real, hits), 0.0, TINY
    e_z = gamma(P + 1) * (np.abs(x) @ np.abs(aux["W"]).T + np.abs(b))
    e_lse = e_z.max(1) + (U * C / np.e + K_EXP * U + gamma(C)) * (1 + gamma(C)) + K_LOG * U * np.log(C) + U * np.abs(lse)
    e_loss_g = np.where(live, e_lse + (e_z * onehot).sum(1) + U * np.abs(aux["loss_g"]), 0.0)
    n = n_real + 1
    bound = e_loss_g.sum() + n * U64 / (1.0 - n * U64) * (np.abs(aux["loss_g"]).sum() + e_loss_g.sum()) + TINY
    return (n_real, hits), float(aux["loss_g"].sum()), float(bound)


def make_case(G, P, C, seed=0):
    """|pooled|, |W|, |bias| <= 1 (W shrinking with the width, as _node_loss_ref.make_case's), targets over the whole class
    range with one outside it where there is room (row 1 of G >= 3: no loss, no hit, counted in totals[0])."""
    rng = np.random.default_rng(seed * 7919 + G * 31 + P * 7 + C)
    pooled = rng.uniform(-1.0, 1.0, (G, P)).astype(np.float32)
    W = (rng.uniform(-1.0, 1.0, (C, P)) / max(1.0, P / 16.0)).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, C).astype(np.float32)
    t = rng.integers(0, C, G).astype(np.int64)
    t[0], t[-1] = 0, C - 1
    if G >= 3:
        t[1] = C
    return dict(pooled=pooled, W=W, bias=b, target=t)


def make_tie_case(G=65, P=65, C=7):
    """Integer-valued pooled and weights, so that every logit is exact in fp32 whatever the order: classes 2 and 5 carry
    the same weights and bias and every other class lies 1000 below them -- the arg-max is class 2, the first of the two.
    Rows target 2 (a hit) and 5 (no hit) in turn."""
    rng = np.random.default_rng(4242)
    pooled = rng.integers(-3, 4, (G, P)).astype(np.float32)
    W = np.zeros((C, P), np.float32)
    W[2] = W[5] = rng.integers(-2, 3, P).astype(np.float32)
    b = np.full(C, -1000.0, np.float32)
    b[2] = b[5] = 3.0
    t = np.where(np.arange(G) % 2 == 0, 2, 5).astype(np.int64)
    return dict(pooled=pooled, W=W, bias=b, target=t)
