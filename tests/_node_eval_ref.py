"""Restatement of the node evaluation head's rule (include/sgx.h, "the node evaluation head") in numpy: sgx_node_loss's
selection, the logits in the stated fp32 order (one correctly rounded fmaf chain over j ascending, then the bias), the
per-row cross entropy in float64 ON those fp32 logits, the arg-max with the first maximum winning, the two-level order of
the double sum, the bound of the kernel's loss_sum derived from its rounding points, the argument errors in their stated
order, and the inputs, the small graph and the loaders the tests run.

u, gamma and the exp / log constants are _train_tail_ref's, fmaf and the arg-max _head_eval_ref's, the selection
_node_loss_ref's.  Nothing here is tuned to what the kernel returns."""
import ctypes

import numpy as np

from _head_eval_ref import argmax_first, fmaf  # noqa: F401  (argmax_first: re-exported for the tests)
from _node_loss_ref import selection
from _train_tail_ref import K_EXP, K_LOG, U, gamma

ROWS = 16                                          # SGX_NODE_LOSS_ROWS
GRID = 512                                         # SGX_NODE_LOSS_GRID
U64 = 2.0 ** -53                                   # float64's unit roundoff: the row losses are added in double
TINY = float(np.finfo(np.float32).tiny)
OK, NULL, SHAPE, UNSUPPORTED, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -7


def logits_f32(H, W, bias):
    """z [n, C] float32 in the rule's order: one fmaf chain from 0 over j ascending of W[c][j] * H[i][j], then + bias[c]."""
    H, W = np.asarray(H, np.float32), np.asarray(W, np.float32)
    (n, P), C = H.shape, W.shape[0]
    z = np.zeros((n, C), np.float32)
    for j in range(P):
        z = fmaf(np.broadcast_to(W[None, :, j], (n, C)), np.broadcast_to(H[:, j, None], (n, C)), z)
    return z if bias is None else (z + np.asarray(bias, np.float32)[None, :]).astype(np.float32)


def row_losses_f64(z32, target):
    """(loss_i, lse, live) per row in float64 from the fp32 logits: m = max, lse = m + log(sum exp(z - m)), loss = lse -
    z[target]; a target outside [0, C) gives 0 and indexes nothing."""
    z = np.asarray(z32, np.float64)
    t = np.asarray(target, np.int64)
    n, C = z.shape
    live = (t >= 0) & (t < C)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    zt = z[np.arange(n), np.where(live, t, 0)]
    return np.where(live, lse - zt, 0.0), lse, live


def sum_in_order(loss, sel):
    """The rule's double sum of the selected rows' losses: per block of ROWS consecutive rows the selected rows added from
    0.0 in ascending row order; the blocks' sums added from 0.0 in ascending block order."""
    loss, sel = np.asarray(loss), np.asarray(sel, bool)
    total = np.float64(0.0)
    for b0 in range(0, loss.shape[0], ROWS):
        s = np.float64(0.0)
        for i in range(b0, min(b0 + ROWS, loss.shape[0])):
            if sel[i]:
                s = s + np.float64(loss[i])
        total = total + s
    return float(total)


def eval_ref(H, W, bias, target, mask=None, n_prefix=None):
    """((M, hits), loss_sum in float64, the bound of the kernel's loss_sum against it, the fp32 logits of every row, and what
    mean_loss_bound needs: the rows' summed fp32 error bound e_rows and the magnitude of the sum).

    hits come from the fp32 logits, as the kernel's do.  The bound, from the rounding points of a selected row with a
    target in range -- the kernel and this reference start from the SAME fp32 logits, so the logits' own error does not
    enter: t_c = z_c - m rounds by u |t_c|, which exp turns into a relative u |t_c| of a term of weight e^t_c / s
    (|t| e^t <= 1 / e, s >= 1: u C / e over the C terms); expf (K_EXP u); the C additions (gamma(C)); logf (K_LOG u log s,
    log s <= log C); m + log s (u |lse|); lse - z_t (u |loss_i|).  The rows' fp32 losses are then added in double: at most
    ROWS additions inside a block, one per block, one into the accumulator: gamma64 of their number times the sum of the
    magnitudes.  With C == 1 the kernel's loss is an exact 0 (expf(0) == 1, logf(1) == 0, m + 0 == m, z - z == 0) and so is
    float64's."""
    H, W = np.asarray(H, np.float32), np.asarray(W, np.float32)
    n, C = H.shape[0], W.shape[0]
    sel = selection(n, mask, n_prefix)
    M = int(sel.sum())
    z32 = logits_f32(H, W, bias)
    if M == 0:
        return (0, 0), 0.0, 0.0, z32, dict(e_rows=0.0, mag=0.0)
    zs = np.where(sel[:, None], z32, np.float32(0.0))        # unselected rows reach nothing, whatever they hold
    loss_i, lse, live = row_losses_f64(zs, target)
    live &= sel
    hits = int((live & (argmax_first(zs) == np.asarray(target, np.int64))).sum())
    if C == 1:
        return (M, hits), 0.0, TINY, z32, dict(e_rows=0.0, mag=0.0)
    e_row = (U * C / np.e + K_EXP * U + gamma(C)) * (1 + gamma(C)) + K_LOG * U * np.log(C) + U * np.abs(lse) + U * np.abs(loss_i)
    e_rows = float(np.where(live, e_row, 0.0).sum())
    n_add = ROWS + -(-n // ROWS) + 1
    mag = float(np.abs(np.where(live, loss_i, 0.0)).sum())
    bound = e_rows + n_add * U64 / (1.0 - n_add * U64) * (mag + e_rows) + TINY
    return (M, hits), sum_in_order(loss_i, live), bound, z32, dict(e_rows=e_rows, mag=mag)


def mean_loss_bound(n, aux):
    """The bound of M * sgx_node_loss's mean loss (fp32, the product formed in double) against eval_ref's loss_sum on the
    same rows: the same fp32 row losses (aux["e_rows"] from float64's), added in fp32 in sgx_node_loss's order -- a loss
    passes ceil(nb / S) + ROWS + S additions (_node_loss_ref.node_bounds) -- and divided by (float)M: gamma of their number
    + 1 times the magnitudes."""
    nb = -(-n // ROWS)
    S = min(nb, GRID)
    n_loss = -(-nb // S) + ROWS + S + 1
    return aux["e_rows"] + gamma(n_loss + 1) * (aux["mag"] + aux["e_rows"]) + TINY


# ---- the inputs of tests/test_gpu_node_eval.py ------------------------------------------------------------------------
ROW_COUNTS = [1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1, GRID * ROWS + 8]      # 1, 15, 16, 17, 33, 8200
WIDTHS = [1, 7, 64, 65]
CLASSES = [1, 2, 7, 64]
MASKS = ["none", "sparse", "zero"]


def prefixes(n):
    """An empty prefix, one that ends inside a block (half the rows, one more where that is a block's edge), the whole
    matrix."""
    mid = n // 2 + (1 if (n // 2) % ROWS == 0 else 0)
    return sorted({0, min(mid, n), n})


def make_case(n, P, C, mask="none", seed=0, bias=True):
    """|H|, |W|, |bias| <= 1 (W shrinking with the width, as _node_loss_ref.make_case's), targets over the whole class range
    with one above it and one below it where there is room (rows 1 and 2: no loss, no hit, counted when selected).  mask:
    "none", "sparse" (about one row in five, with a whole block of ROWS rows unselected where there are three blocks),
    "zero" (no row)."""
    rng = np.random.default_rng(seed * 7919 + n * 31 + P * 7 + C)
    H = rng.uniform(-1.0, 1.0, (n, P)).astype(np.float32)
    W = (rng.uniform(-1.0, 1.0, (C, P)) / max(1.0, P / 16.0)).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, C).astype(np.float32) if bias else None
    t = rng.integers(0, C, n).astype(np.int64)
    t[0], t[-1] = 0, C - 1
    if n >= 3:
        t[1] = C
    if n >= 4:
        t[2] = -1
    m = None
    if mask == "sparse":
        m = rng.random(n) < 0.2
        m[0] = True
        if n >= 4:
            m[1] = m[2] = True                               # the rows whose targets lie outside the range count
        if n >= 3 * ROWS:
            m[ROWS:2 * ROWS] = False
    elif mask == "zero":
        m = np.zeros(n, bool)
    elif mask != "none":
        raise ValueError(mask)
    return dict(H=H, W=W, bias=b, target=t, mask=m)


def gpu_case_specs():
    """(id, make_case arguments) of the kernel test: every row count at P = 7, C = 5; every width and class count at 33
    rows; each with every mask; no bias at two shapes."""
    specs = []
    for n in ROW_COUNTS:
        for mask in MASKS:
            specs.append((f"rows{n}-{mask}", dict(n=n, P=7, C=5, mask=mask)))
    for P in WIDTHS:
        for C in CLASSES:
            for mask in MASKS:
                specs.append((f"P{P}-C{C}-{mask}", dict(n=2 * ROWS + 1, P=P, C=C, mask=mask, seed=1)))
    specs.append(("no-bias", dict(n=2 * ROWS + 1, P=65, C=7, mask="sparse", seed=2, bias=False)))
    specs.append(("no-bias-past-the-grid", dict(n=GRID * ROWS + 8, P=7, C=2, mask="none", seed=3, bias=False)))
    return specs


def make_tie_case(n=2 * ROWS + 1, P=7, C=7):
    """Integer-valued H and weights, so that every logit is exact in fp32: classes 2 and 5 carry the same weights and bias
    and every other class lies 1000 below them -- the arg-max is class 2, the first of the two.  Rows target 2 (a hit) and
    5 (no hit) in turn."""
    rng = np.random.default_rng(4242)
    H = rng.integers(-3, 4, (n, P)).astype(np.float32)
    W = np.zeros((C, P), np.float32)
    W[2] = W[5] = rng.integers(-2, 3, P).astype(np.float32)
    b = np.full(C, -1000.0, np.float32)
    b[2] = b[5] = 3.0
    t = np.where(np.arange(n) % 2 == 0, 2, 5).astype(np.int64)
    return dict(H=H, W=W, bias=b, target=t, mask=None)


# ---- the argument errors, in the header's order: every refusal returns before a launch -------------------------------------
def check_argument_errors(lib):
    """Calls sgx_node_eval through the C ABI with host addresses that are never dereferenced."""
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p(base)                                # stands for every operand
    ws, wsb = ctypes.c_void_p(base), 4096

    def call(n=40, n_prefix=40, P=8, C=2, H=p, W=p, bias=p, target=p, mask=None, totals=p, loss_sum=p, logits=None, ws=ws, wsb=wsb):
        return lib.sgx_node_eval(n, n_prefix, P, C, H, W, bias, target, mask, totals, loss_sum, logits, ws, wsb, None)

    size = lib.sgx_node_eval_workspace_bytes
    need = size(40, 40, 8, 2)
    assert need == 256 + 256 and size(40, 0, 8, 2) == 256 and size(40, -3, 8, 2) == 256      # 3 blocks of 16 bytes; none
    assert size(8200, 8200, 1, 1) == 256 + 8448 and size(8200, 17, 1, 1) == 256 + 256 and size(17, 8200, 1, 1) == 256 + 256
    for bad in (dict(n=0, n_prefix=0), dict(n_prefix=-1), dict(P=0), dict(C=0)):
        assert call(**bad) == SHAPE, bad
    assert call(n=0, H=None) == SHAPE and call(H=None, P=2000) == NULL                       # the order of the checks
    for field in ("H", "W", "target", "totals", "loss_sum"):
        assert call(**{field: None}) == NULL, field
    assert call(bias=None, ws=None) == WORKSPACE                                            # (bias and mask may be NULL)
    # sgx_node_loss's limits
    assert call(P=1025) == UNSUPPORTED and call(C=65) == UNSUPPORTED and call(P=1024, C=17) == UNSUPPORTED
    assert call(P=1025, ws=None) == UNSUPPORTED
    assert size(40, 40, 1025, 2) == 0 and size(40, 40, 8, 65) == 0 and size(40, 40, 1024, 17) == 0 and size(0, 0, 8, 2) == 0
    assert size(40, 40, 1024, 16) == need and size(40, 40, 256, 64) == need
    assert call(ws=None) == WORKSPACE and call(wsb=need - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(base + 64)) == ALIGN
    assert call(ws=ctypes.c_void_p(base + 64), wsb=need - 1) == WORKSPACE
    # an empty prefix and no logits wanted: a valid call that launches nothing
    assert call(n_prefix=0) == OK


# ---- the small graph and the loaders of the trainer tests ---------------------------------------------------------------
N_NODES, N_FEATURES, N_CLASSES, HIDDEN = 240, 40, 5, 16
BATCH, FANOUTS, N_TEST, N_TRAIN = 32, [3, 2], 70, 70         # the test set: two full batches and a short one of 6 seeds


def small_graph():
    """(x [240, 40] float32 with about a third of its entries set, edge_index [2, E] int64 with repeated edges and some
    stored loops, y [240] int64, train_mask, test_mask: 70 nodes each, disjoint), numpy arrays."""
    rng = np.random.default_rng(8)
    n = N_NODES
    m = rng.random((n, n)) < 0.03
    np.fill_diagonal(m, rng.random(n) < 0.2)
    src, dst = np.nonzero(m)
    rep = rng.integers(1, 4, len(src))
    ei = np.stack([np.repeat(src, rep), np.repeat(dst, rep)]).astype(np.int64)
    x = ((rng.random((n, N_FEATURES)) < 0.3) * rng.random((n, N_FEATURES))).astype(np.float32)
    x[3] = 0                                                 # an empty feature row
    y = (np.arange(n) * 7 % N_CLASSES).astype(np.int64)
    order = rng.permutation(n)
    train, test = np.zeros(n, bool), np.zeros(n, bool)
    train[order[:N_TRAIN]] = True
    test[order[N_TRAIN:N_TRAIN + N_TEST]] = True
    return x, ei, y, train, test


def node_data(device):
    """The small graph as a pyg_lite.NodeData on `device`."""
    import torch
    from sgracex1_amd import pyg_lite
    x, ei, y, train, test = small_graph()
    t = lambda a: torch.from_numpy(a).to(device)
    return pyg_lite.NodeData(t(x).contiguous(), t(ei), t(y), train_mask=t(train), test_mask=t(test))


def loader_kwargs(gat, half, split="test", shuffle=False):
    """The NeighborLoader arguments of a configuration (attention: fill = 1, so that no live row is dead -- a dead row's
    uniform softmax spans the padded width, the one documented difference of a padded batch) over the test or the training
    nodes; the training loader of an attention model is transposed, what capture_loader asks for."""
    import torch
    return dict(batch_size=BATCH, shuffle=shuffle, seed=3, prepare="sym_norm2", fill=1 if gat else 0,
                dtype=torch.float16 if half else torch.float32, transposed=bool(gat) and split == "train", pad=True)
