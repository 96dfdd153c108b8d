"""The reference's layer backward restated in float64, for the gradient tests.

FPYNQ_GAT.backward of demo/sgrace_lib/sgrace.py (SG.py below), the `accb == 0` branch, SG.py:884-1126, with what its
forward saves for it (SG.py:678-680: the UNquantised adjacency, e and the attention matrix), and FPYNQ.backward of the
molecule notebook (MOL cell 16).  Written from the formulas:

    GAT   so = g Wh^T;  dx = P * so;  sg = dx - P * rowsum(dx)          softmax backward over all N columns
          sg = where(adj > 0, sg, 0)                                    mask on the unquantised values (SG.py:1009)
          sg = (e > 0 ? 1 : alpha) * sg                                 LeakyReLU slope
          grad_attention = [Wh^T rowsum(sg) ; Wh^T colsum(sg)]
    both  grad_input = P (g W^T);  grad_weights = X^T (P g)             P and not P^T, as the reference
    GCN   (compute_attention = 0) P = the unquantised adjacency, grad_attention = 0
    MOL   grad_W = X^T A g;  grad_x = A g W^T                           (= the GCN form)

with Wh = X W unquantised (SG.py:1012-1017) and, for GAT, P = the forward's softmax: S on the stored entries of a
live row, 1/N on EVERY column of a dead row -- a row the forward found without a positive entry in the adjacency it
masked with (SG.py:638-641; the quantised one in quantised mode).  Like the reference, deq_o and the layer's ReLU
play no part (RPYNQ masks the gradient, not this Function).

Two forms give the same numbers: `dense` builds N x N matrices (keep N <= ~4 K), `edges` works on the edge list and
states the dead rows in closed form (mean of g for P g, g_i . colsum(Wh) / N for the softmax row sum).  Each returns
the three gradients and, from the same formulas on absolute values (|X| |W| for Wh), an element-wise magnitude bound
that the rounding error of an fp32 evaluation is measured against.

The adjacency is (rowptr, col, val) as stored (fp16 values when the layer stores fp16); E and S are the forward's
per-entry scores and softmax weights; every tensor may live on the CPU or the GPU.
"""
import torch

D = torch.float64


def _rows(rowptr, nnz):
    deg = (rowptr[1:] - rowptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(deg.numel(), device=rowptr.device), deg, output_size=nnz)


def _prep(rowptr, col, val, X, W, g):
    rowptr = rowptr.long()
    nnz = int(rowptr[-1])
    return (rowptr, _rows(rowptr, nnz), col[:nnz].long(), val[:nnz].to(D), X.to(D), W.to(D), g.to(D))


def dense(rowptr, col, val, X, W, g, gat=False, E=None, S=None, dead=None, alpha=0.2):
    """N x N form.  -> (grads, bounds), dicts with grad_input, grad_weights and (gat) grad_attention."""
    rowptr, row, col, val, X, W, g = _prep(rowptr, col, val, X, W, g)
    n, n_cols = rowptr.numel() - 1, X.shape[0]
    dev = X.device

    def scatter(v):
        m = torch.zeros((n, n_cols), dtype=D, device=dev)
        return m.index_put_((row, col), v.to(D), accumulate=True)

    A = scatter(val)
    Wh, Wha = X @ W, X.abs() @ W.abs()
    grads, bounds = {}, {}
    if gat:
        P = scatter(S)
        P[dead] = 1.0 / n_cols
        keep = A > 0
        slope = torch.where(scatter(E) > 0, torch.ones_like(A), torch.full_like(A, alpha))
        for key, p, wh, gg, sign in (("v", P, Wh, g, -1.0), ("b", P.abs(), Wha, g.abs(), 1.0)):
            dx = p * (gg @ wh.t())
            sg = torch.where(keep, dx + sign * p * dx.sum(1, keepdim=True), torch.zeros_like(dx)) * slope
            ga = torch.cat([wh.t() @ sg.sum(1), wh.t() @ sg.sum(0)]).unsqueeze(1)
            (grads if key == "v" else bounds)["grad_attention"] = ga
    else:
        P = A
    grads["grad_input"] = P @ (g @ W.t())
    grads["grad_weights"] = X.t() @ (P @ g)
    bounds["grad_input"] = P.abs() @ (g.abs() @ W.abs().t())
    bounds["grad_weights"] = X.abs().t() @ (P.abs() @ g.abs())
    return grads, bounds


def _spmm(row, col, w, H, n, chunk=1 << 16):
    """sum over the entries of a row of w_e H[col_e], in chunks of entries"""
    out = torch.zeros((n, H.shape[1]), dtype=D, device=H.device)
    for i in range(0, row.numel(), chunk):
        out.index_add_(0, row[i:i + chunk], w[i:i + chunk, None] * H[col[i:i + chunk]])
    return out


def _dots(row, col, G, H, chunk=1 << 16):
    """G[row_e] . H[col_e] for every entry"""
    return torch.cat([(G[row[i:i + chunk]] * H[col[i:i + chunk]]).sum(1) for i in range(0, row.numel(), chunk)]
                     or [torch.zeros(0, dtype=D, device=G.device)])


def edges(rowptr, col, val, X, W, g, gat=False, E=None, S=None, dead=None, alpha=0.2):
    """Edge-list form of `dense`, same results; dead rows in closed form."""
    rowptr, row, col, val, X, W, g = _prep(rowptr, col, val, X, W, g)
    n, n_cols = rowptr.numel() - 1, X.shape[0]
    Wh, Wha = X @ W, X.abs() @ W.abs()
    grads, bounds = {}, {}
    if gat:
        assert n == n_cols, "a dead row's softmax runs over the N nodes: square adjacency"
        dead = dead.to(torch.bool)
        dead_e = dead[row]
        P = torch.where(dead_e, torch.full_like(val, 1.0 / n_cols), S.to(D)[:row.numel()])
        keep = val > 0
        slope = torch.where(E.to(D)[:row.numel()] > 0, torch.ones_like(val), torch.full_like(val, alpha))
        for key, p, wh, gg, sign in (("v", P, Wh, g, -1.0), ("b", P.abs(), Wha, g.abs(), 1.0)):
            dx = p * _dots(row, col, gg, wh)
            rs = torch.zeros(n, dtype=D, device=X.device).index_add_(0, row, dx)
            rs = torch.where(dead, gg @ wh.sum(0) / n_cols, rs)           # sum over all N columns of 1/N g_i . Wh_k
            sg = torch.where(keep, dx + sign * p * rs[row], torch.zeros_like(dx)) * slope
            g1 = torch.zeros(n, dtype=D, device=X.device).index_add_(0, row, sg)
            g2 = torch.zeros(n_cols, dtype=D, device=X.device).index_add_(0, col, sg)
            (grads if key == "v" else bounds)["grad_attention"] = torch.cat([wh.t() @ g1, wh.t() @ g2]).unsqueeze(1)
    else:
        P = val
        dead = torch.zeros(n, dtype=torch.bool, device=X.device)
    for key, p, gg, w, x in (("v", P, g, W, X), ("b", P.abs(), g.abs(), W.abs(), X.abs())):
        pg = _spmm(row, col, p, gg, n)
        pg = torch.where(dead[:, None], gg.sum(0, keepdim=True) / n_cols, pg)     # a dead row of P: 1/N everywhere
        out = grads if key == "v" else bounds
        out["grad_input"] = pg @ w.t()
        out["grad_weights"] = x.t() @ pg
    return grads, bounds


TINY = 1e-3          # positive, below half a grid step of the adjacency at every width (a_s >= 1/255): quantises to 0


def masked_graph(n, seed, density=0.15):
    """A graph with every kind of row the GAT mask treats differently, built dense (n of a few thousand at most).
    -> (rowptr int64, col int64, val fp32, rows: kind -> row index), on the CPU"""
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand((n, n), generator=g) < density).float()
    a = ((a + a.t() + torch.eye(n)) > 0).float()
    deg = a.sum(1)
    a = a / torch.sqrt(deg[:, None] * deg[None, :])
    stored = a != 0
    rows = dict(empty=3, non_positive=5, tiny=8, tiny_entry=10)
    stored[rows["empty"]] = False                                   # no entry at all
    vals = a.clone()
    r = rows["non_positive"]
    vals[r] = torch.where(stored[r], -vals[r], vals[r])             # entries, none positive, one an explicit zero
    first = int(stored[r].nonzero()[0])
    vals[r, first] = 0.0
    r = rows["tiny"]
    vals[r] = torch.where(stored[r], torch.full_like(vals[r], TINY), vals[r])   # positive, all quantise to 0
    r = rows["tiny_entry"]
    vals[r, int(stored[r].nonzero()[-1])] = TINY                    # a live row with one entry that quantises to 0
    idx = stored.nonzero().t()                                      # sorted by (row, col)
    val = vals[idx[0], idx[1]]
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(idx[0], minlength=n), 0)
    return rowptr, idx[1], val, rows


def dead_rows_of(rowptr, val):
    """Rows with no positive value (SG.py:640 `adj > 0` leaves them without a neighbour)."""
    rowptr = rowptr.long()
    row = _rows(rowptr, int(rowptr[-1]))
    live = torch.zeros(rowptr.numel() - 1, dtype=torch.int64, device=val.device)
    live.index_add_(0, row, (val[:row.numel()] > 0).long())
    return live == 0


def worst(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0): the error in units of the magnitude bound."""
    err = (got.to(D) - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


def check(got, grads, bounds, tol, what=""):
    """Every gradient in `got` (name -> tensor) within tol (a number, or name -> number) x its magnitude bound;
    returns name -> worst ratio."""
    figures = {}
    for name, t in got.items():
        want = grads[name]
        assert tuple(t.shape) == tuple(want.shape), (what, name, tuple(t.shape), tuple(want.shape))
        assert torch.isfinite(t).all(), (what, name)
        figures[name] = worst(t, want, bounds[name])
    tols = tol if isinstance(tol, dict) else {k: tol for k in figures}
    bad = {k: v for k, v in figures.items() if not v <= tols[k]}
    assert not bad, (what, bad, tol)
    return figures
