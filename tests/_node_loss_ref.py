"""Restatement of the node loss head's rule (include/sgx.h, "the node loss head") in numpy float64, the error bounds of the
fp32 kernel derived from its operation counts and the summation order the header writes down, and the inputs the GPU
tests run (tests/test_node_loss_cpu.py holds every one of them to the conditions the bounds need).

The dropout mask, gamma and the exp / log constants are _train_tail_ref's.  Nothing here is tuned to what the kernel
returns."""
import numpy as np

from _train_tail_ref import K_EXP, K_LOG, U, dropped, gamma, keep_mask  # noqa: F401  (keep_mask: re-exported for the tests)

ROWS = 16                    # SGX_NODE_LOSS_ROWS
GRID = 512                   # SGX_NODE_LOSS_GRID
TINY = float(np.finfo(np.float32).tiny)


def selection(n, mask=None, n_prefix=None):
    sel = np.arange(n) < (n if n_prefix is None else n_prefix)
    if mask is not None:
        sel &= np.asarray(mask).astype(np.uint8) != 0
    return sel


def node_f64(H, W, bias, target, mask=None, n_prefix=None, p=0.0, seed=0, step=0, grad_scale=1.0):
    """loss, logits, grad_H, grad_W, grad_bias (None without a bias), counts = (M, hits) in float64 from the fp32 inputs,
    plus what the bounds need."""
    x32, keep, scale = dropped(H, p, seed, step)
    x, W = x32.astype(np.float64), np.asarray(W, np.float64)
    n, P = x.shape
    C = W.shape[0]
    b = np.zeros(C) if bias is None else np.asarray(bias, np.float64)
    t = np.asarray(target, np.int64)
    sel = selection(n, mask, n_prefix)
    M = int(sel.sum())
    live = sel & (t >= 0) & (t < C)
    z = x @ W.T + b
    m = z.max(1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
    onehot = np.zeros((n, C))
    onehot[np.nonzero(live)[0], t[live]] = 1.0
    loss_i = np.where(live, lse - (z * onehot).sum(1), 0.0)
    prob = np.exp(z - lse[:, None])
    gs = float(np.float32(grad_scale)) / M if M else 0.0
    dz = np.where(live[:, None], (prob - onehot) * gs, 0.0)
    grad_H = np.where(keep & sel[:, None], float(scale) * (dz @ W), 0.0)
    grad_W = dz.T @ x
    grad_b = None if bias is None else dz.sum(0)
    hits = int((live & (z.argmax(1) == t)).sum())          # numpy's arg-max: the lowest index of the maximum
    loss = loss_i.sum() / M if M else 0.0
    aux = dict(x=x, keep=keep, scale=float(scale), z=z, lse=lse, prob=prob, onehot=onehot, live=live, sel=sel, dz=dz, gs=gs,
               loss_i=loss_i, W=W, b=b, M=M)
    return loss, z, grad_H, grad_W, grad_b, (M, hits), aux


def node_bounds(aux):
    """Absolute error bounds of sgx_node_loss against node_f64, per output, from the header's summation order:
      logits   one fmaf chain of P terms, then the bias: gamma(P + 1) (|W| |x| + |b|)
      lse, loss_i, dz   as _train_tail_ref.head_bounds derives them (the same operations per row)
      loss     a loss_i passes ceil(nb / S) additions of its row position's chain, ROWS additions over the positions, S over
               the slices, and the division by (float)M (exact for M < 2^24): gamma of their number + 1
      grad_H   C fmafs and the scale: gamma(C + 1), plus |W|^T E_dz, times scale
      grad_W   a term passes at most ROWS ceil(nb / S) fmafs of its slice's chain and S additions: gamma(that + 1);
      grad_bias   the same count of additions
    With C == 1 every row has lse == z exactly (expf(0) == 1, logf(1) == 0, m + 0 == m), so loss_i and dz are exact zeros
    on the device as in float64: loss and the gradients get the bound TINY alone."""
    x, z, lse, prob, onehot, dz, gs, W, b = (aux[k] for k in ("x", "z", "lse", "prob", "onehot", "dz", "gs", "W", "b"))
    n, P = x.shape
    C = W.shape[0]
    live, M = aux["live"], aux["M"]
    e_z = gamma(P + 1) * (np.abs(x) @ np.abs(W).T + np.abs(b))
    if C == 1 or M == 0:
        zero = lambda a: np.zeros_like(a) + TINY
        return dict(logits=e_z + TINY, loss=TINY, grad_H=zero(x), grad_W=zero(W), grad_bias=zero(b))
    e_lse = e_z.max(1) + (U * C / np.e + K_EXP * U + gamma(C)) * (1 + gamma(C)) + K_LOG * U * np.log(C) + U * np.abs(lse)
    e_loss_i = np.where(live, e_lse + (e_z * onehot).sum(1) + U * np.abs(aux["loss_i"]), 0.0)
    nb = -(-n // ROWS)
    S = min(nb, GRID)
    per_slice = -(-nb // S)
    n_loss = per_slice + ROWS + S
    e_loss = e_loss_i.sum() / M + gamma(n_loss + 1) * np.abs(aux["loss_i"]).sum() / M
    d_arg = e_z + e_lse[:, None] + U * np.abs(z - lse[:, None])
    e_prob = prob * (np.expm1(d_arg) + K_EXP * U * np.exp(d_arg))
    e_dz = np.where(live[:, None], gs * (e_prob + U * np.abs(prob - onehot)) * (1 + 3 * U) + 3 * U * np.abs(dz), 0.0)
    scale = aux["scale"]
    e_gh = np.where(aux["keep"], scale * (e_dz @ np.abs(W) + gamma(C + 1) * (np.abs(dz) @ np.abs(W))) * (1 + U), 0.0)
    n_sum = ROWS * per_slice + S
    e_gw = e_dz.T @ np.abs(x) + gamma(n_sum + 1) * (np.abs(dz).T @ np.abs(x))
    e_gb = e_dz.sum(0) + gamma(n_sum + 1) * np.abs(dz).sum(0)
    return dict(logits=e_z + TINY, loss=e_loss + TINY, grad_H=e_gh + TINY, grad_W=e_gw + TINY, grad_bias=e_gb + TINY)


def top_two_gap(z):
    """The gap between the largest and the second largest logit of every row (inf with one class)."""
    if z.shape[1] == 1:
        return np.full(z.shape[0], np.inf)
    s = np.sort(z, axis=1)
    return s[:, -1] - s[:, -2]


# ---- the inputs of tests/test_gpu_node_loss.py ---------------------------------------------------------------------------
def make_case(n, P, C, select="mask", p=0.5, seed=0, bias=True, grad_scale=1.0, ties=False):
    """|H|, |W|, |bias| <= 1, W strictly positive (so that grad_H's zero pattern shows the dropout mask: see the GPU test),
    targets over the whole class range.  select: "none" (no mask, no prefix), "all", "empty", "one", "hole" (a whole block
    unselected between two selected ones), "prefix0", "prefixR1", "prefix+mask", "mask" (a random half).
    ties: rows 1 and 2 of H are zero and the bias holds its maximum twice (classes 1 and C - 1), so their logits are the
    bias exactly: the arg-max is class 1; row 1 targets C - 1 (no hit), row 2 targets 1 (a hit).  Needs p == 0, C >= 3."""
    rng = np.random.default_rng(seed * 7919 + n * 31 + P * 7 + C)
    H = rng.uniform(-1.0, 1.0, (n, P)).astype(np.float32)
    # W shrinks with the width: the logits' bound grows as P sum |W| |x|, and a softmax that saturates leaves gradients
    # that cancel to less than a hundred times that bound
    W = (rng.uniform(0.05, 1.0, (C, P)) / max(1.0, P / 16.0)).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, C).astype(np.float32) if bias else None
    t = rng.integers(0, C, n)
    t[0], t[-1] = 0, C - 1
    mask, n_prefix = None, None
    if select == "all":
        mask = np.ones(n, bool)
    elif select == "empty":
        mask = np.zeros(n, bool)
    elif select == "one":
        mask = np.zeros(n, bool)
        mask[n // 2] = True
    elif select == "hole":
        mask = np.ones(n, bool)
        mask[ROWS:2 * ROWS] = False
    elif select == "prefix0":
        n_prefix = 0
    elif select == "prefixR1":
        n_prefix = min(n, ROWS + 1)
    elif select == "prefix+mask":
        mask, n_prefix = rng.random(n) < 0.5, min(n, ROWS + 1)
    elif select == "mask":
        mask = rng.random(n) < 0.5
        mask[0] = True
    elif select != "none":
        raise ValueError(select)
    tie_rows = []
    if ties:
        assert p == 0.0 and C >= 3 and n >= 3 and bias
        H[1:3] = 0.0
        b[:] = rng.uniform(-1.0, 0.0, C).astype(np.float32)
        b[1] = b[C - 1] = np.float32(0.5)
        t[1], t[2] = C - 1, 1
        if mask is not None:
            mask[1:3] = True
        tie_rows = [1, 2]
    return dict(H=H, W=W, bias=b, target=t.astype(np.int64), mask=mask, n_prefix=n_prefix, p=p, seed=1000 + seed, step=3 + seed,
                grad_scale=grad_scale, tie_rows=tie_rows)


R, S = ROWS, GRID
ROW_COUNTS = [1, R - 1, R, R + 1, 3 * R + 5]
WIDTHS = [1, 63, 64, 65, 256, 1024]
CLASSES = [1, 2, 7, 64]
SELECTIONS = ["none", "all", "empty", "one", "hole", "prefix0", "prefixR1", "prefix+mask"]


def gpu_case_specs():
    """(id, make_case arguments) of every case of the GPU test: the row counts at P = 7, C = 5 with a random mask; the
    widths and class counts at 3 R + 5 rows within C P <= 16384; C P = 16384 itself; two blocks in one slice; every
    selection; no bias; a gradient scale; the ties."""
    specs = []
    for n in ROW_COUNTS:
        for p in (0.0, 0.5):
            specs.append((f"rows{n}-p{p}", dict(n=n, P=7, C=5, select="mask", p=p)))
    for P in WIDTHS:
        for C in CLASSES:
            if C * P <= 16384:
                specs.append((f"P{P}-C{C}", dict(n=3 * R + 5, P=P, C=C, select="mask", p=0.5, seed=1)))
    specs.append(("CP16384", dict(n=R + 1, P=256, C=64, select="mask", p=0.5, seed=2)))
    specs.append(("two-blocks-a-slice", dict(n=S * R + R + 1, P=3, C=2, select="mask", p=0.5, seed=3)))
    for sel in SELECTIONS:
        for p in (0.0, 0.9):
            specs.append((f"sel-{sel}-p{p}", dict(n=3 * R + 5, P=65, C=7, select=sel, p=p, seed=4)))
    specs.append(("no-bias", dict(n=3 * R + 5, P=64, C=7, select="mask", p=0.5, seed=15, bias=False)))
    specs.append(("grad-scale", dict(n=3 * R + 5, P=64, C=7, select="mask", p=0.5, seed=6, grad_scale=0.37)))
    specs.append(("ties", dict(n=3 * R + 5, P=64, C=7, select="hole", p=0.0, seed=7, ties=True)))
    return specs
