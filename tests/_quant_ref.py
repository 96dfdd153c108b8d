"""The quantised layer (oracle/quant_oracle.py::layer, SG.py:565-667) restated on CSR operands, so that it runs at the
10^4..10^5 rows where the kernels change path and the oracle's dense N x N form cannot, plus the operands the path
tests run it on and the comparison they use.

Stage 1, H = requant(X_q . W_q), is EXACT.  A quantised operand is an integer code over a power of two (value =
code / den, den = 2^(w_qbits-1), 2 at one bit), so a product of two is an integer over den^2 and a row's sum is an
integer over den^2 -- which fp32 holds exactly, partial sums in any order included, while sum |code_x| |code_w| stays
below 2^24.  stage1() forms the code sums in int64, converts them to float32 and applies the oracle's three lines
(/ 2^scale_fea, clip, torch.round(decimals = iq - 1)) in torch CPU float32, whose bits the kernels' epilogue matches
(tests/test_gpu_quant.py::test_requantize_bit_exact).  It returns the largest row sum of |code_x| |code_w| with H: the
claim holds only where that is below 2^24, and every caller asserts so from its own operands.

Stage 2 is float64 on the GIVEN fp32 H (stage 1's rounding does not leak into it) with a derived bound:
    GCN  D = relu(A_q . H) deq_o,   |dD_ij| <= (deg_i + 3) 2^-24 |deq_o| sum_e |a_e| |H[c_e, j]|
         -- an fp32 sum of deg_i products in any order (fma chain, lane tree or task partials), the ReLU (exact), the
         scale (one rounding) and one to spare; no measured constant.
    GAT  tests/_gat_ref.py::forward on the quantised attention, the given H as Wh and live = (A_q > 0); D and its
         bound times |deq_o|.
deq_o is the fp32 number the library is handed (struct sgx_quant holds a float).
"""
import numpy as np
import torch

import _gat_ref as R
from oracle import quant_oracle as QO

U = 2.0 ** -24
EXACT_BELOW = 1 << 24


def den(bits):
    return 2 if bits == 1 else 2 ** (bits - 1)


def quantise(x, signed, c):
    """float32 values on their grid (the oracle's own functions) and their integer codes (int64)."""
    x = torch.as_tensor(np.asarray(x, np.float32)).clone()
    if signed:
        q = QO.quantization_fbits(x, c.w_s, c.w_z, c.w_qbits)
    else:
        q = QO.quantization_ufbits(x, c.f_s, c.f_z, c.w_qbits)
    q = q.numpy().astype(np.float32)
    code = np.rint(q.astype(np.float64) * den(c.w_qbits)).astype(np.int64)
    assert np.array_equal((code / den(c.w_qbits)).astype(np.float32), q)
    return q, code


def quantise_adj(val, c):
    v = torch.as_tensor(np.asarray(val, np.float32)).clone()
    return QO.quantization_ufbits(v, c.a_s, c.a_z, c.w_qbits).numpy().astype(np.float32)


def csr_matmul(rowptr, col, val, T):
    """sum_e val_e T[col_e, :] per row, in the type of val / T (int64: exact; float64), a block of rows at a time."""
    rowptr = np.asarray(rowptr, np.int64)
    n, P = len(rowptr) - 1, T.shape[1]
    out = np.zeros((n, P), dtype=np.result_type(val.dtype, T.dtype))
    budget = max(1, (1 << 22) // max(P, 1))                       # entries per block
    r0 = 0
    while r0 < n:
        r1 = int(np.searchsorted(rowptr, rowptr[r0] + budget, side="right")) - 1
        r1 = min(max(r1, r0 + 1), n)
        e0, e1 = rowptr[r0], rowptr[r1]
        if e1 > e0:
            prod = val[e0:e1, None] * T[col[e0:e1]]
            starts = rowptr[r0:r1] - e0
            nonempty = np.diff(rowptr[r0:r1 + 1]) > 0
            out[r0:r1][nonempty] = np.add.reduceat(prod, starts[nonempty], axis=0)
        r0 = r1
    return out


def take_rows(rowptr, col, val, rows):
    """The CSR of the listed rows alone (same columns)."""
    rowptr = np.asarray(rowptr, np.int64)
    deg = rowptr[rows + 1] - rowptr[rows]
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum(deg)
    idx = np.repeat(rowptr[rows] - rp[:-1], deg) + np.arange(rp[-1])
    return rp, col[idx], val[idx]


def requant(h32, c, mutant=None):
    """SG.py:607-616 on float32 sums: the oracle's three lines in torch CPU float32.  Returns (H, facts)."""
    iq = c.internal_quantization
    Wh = torch.as_tensor(h32)
    if mutant == "no_requant":
        return Wh.numpy().copy(), dict(clip_hi=0, clip_lo=0, rounded=0)
    Wh = Wh / (2 ** c.scale_fea)
    a_max = (2 ** iq - 1) / (2 ** iq)
    clipped = Wh if mutant == "no_clip" else torch.clip(Wh, min=-a_max, max=a_max)
    out = torch.round(clipped, decimals=iq - 1)
    facts = dict(clip_hi=int((Wh > a_max).sum()), clip_lo=int((Wh < -a_max).sum()), rounded=int((out != clipped).sum()))
    return out.numpy(), facts


def stage1(X, W, c, rows=None, mutant=None):
    """H = requant(X_q . W_q) exactly.  X: a dense [n, M] array or a CSR triple (rowptr, col, val); W [M, P];
    rows: the rows wanted (all).  Returns (H float32 [rows, P], max over those rows of sum |code_x| |code_w|, facts)."""
    _wq, cw = quantise(W, 1, c)
    if isinstance(X, tuple):
        rowptr, col, val = X
        col = np.asarray(col, np.int64)
        _xq, cx = quantise(val, 0, c)
        if rows is not None:
            rowptr, col, cx = take_rows(rowptr, col, cx, np.asarray(rows, np.int64))
        sums = csr_matmul(rowptr, col, cx, cw)
        mag = csr_matmul(rowptr, col, np.abs(cx), np.abs(cw))
    else:
        X = np.asarray(X, np.float32)
        _xq, cx = quantise(X if rows is None else X[np.asarray(rows, np.int64)], 0, c)
        # (float64 holds these integers exactly -- far below 2^53 -- and its product runs through BLAS)
        sums = (cx.astype(np.float64) @ cw.astype(np.float64)).astype(np.int64)
        mag = (np.abs(cx).astype(np.float64) @ np.abs(cw).astype(np.float64)).astype(np.int64)
    magnitude = int(mag.max()) if mag.size else 0
    h32 = sums.astype(np.float32) / np.float32(den(c.w_qbits) ** 2)            # exact below 2^24: a power-of-two divisor
    H, facts = requant(h32, c, mutant)
    return H, magnitude, facts


def deq32(c):
    return float(np.float32(c.deq_o))


def stage2_gcn(adj, aq, H, c, relu, mutant=None):
    """D = relu(A_q . H) deq_o in float64 from the given fp32 H, and the element-wise bound.  adj = (rowptr, col)."""
    rowptr, col = np.asarray(adj[0], np.int64), np.asarray(adj[1], np.int64)
    a, H64, dq = np.asarray(aq, np.float64), np.asarray(H, np.float64), deq32(c)
    s = csr_matmul(rowptr, col, a, H64)
    mag = csr_matmul(rowptr, col, np.abs(a), np.abs(H64))
    if mutant == "scale_before_relu":
        D = np.maximum(s * dq, 0.0) if relu else s * dq
    else:
        D = (np.maximum(s, 0.0) if relu else s) * dq
    if mutant == "scale_twice":
        D = D * dq
    bound = (np.diff(rowptr)[:, None] + 3) * U * abs(dq) * mag
    return D, bound


def stage2_gat(adj, aq, H, att_q, c, relu, dead_rule, mutant=None, alpha=0.2):
    """_gat_ref.forward on the quantised operands, D and its bound times |deq_o|.  Returns (D, bound, ref)."""
    g = dict(rowptr=np.asarray(adj[0], np.int64), col=np.asarray(adj[1], np.int64), val=np.asarray(aq, np.float64),
             Wh=np.asarray(H, np.float64), att=np.asarray(att_q, np.float64).reshape(-1))
    dq = deq32(c)
    pre = relu and mutant != "scale_before_relu"
    ref = R.forward(g, 1, alpha=alpha, relu=pre, dead_rule=dead_rule, out="f32", live=g["val"] > 0)
    D, bound = ref["D"] * dq, ref["bD"] * abs(dq)
    if mutant == "scale_before_relu" and relu:
        D = np.maximum(D, 0.0)
    if mutant == "scale_twice":
        D = D * dq
    if mutant == "fill_unscaled":
        D[ref["dead"]] = ref["D"][ref["dead"]]
    return D, bound, ref


def layer(adj, a_val, X, W, att, c, relu, gat, dead_rule="mean", mutant=None):
    """The whole layer on CSR operands: adj = (rowptr, col), a_val its unquantised values; X dense or a CSR triple;
    W [M, P]; att [2P] (GAT).  Returns dict(H, magnitude, facts, D, bound, aq)."""
    H, magnitude, facts = stage1(X, W, c, mutant=mutant)
    aq = quantise_adj(a_val, c)
    if gat:
        att_q, _ = quantise(np.asarray(att, np.float32).reshape(-1), 1, c)
        D, bound, ref = stage2_gat(adj, aq, H, att_q, c, relu, dead_rule, mutant)
        dead = ref["dead"]
    else:
        D, bound = stage2_gcn(adj, aq, H, c, relu, mutant)
        dead = None
    return dict(H=H, magnitude=magnitude, facts=facts, D=D, bound=bound, aq=aq, dead=dead)


# ---- the comparison the GPU tests use ---------------------------------------------------------------------------------

def check_H(got, want, magnitude):
    """Bit for bit -- allowed only where the exactness condition holds (a condition on the inputs, asserted first)."""
    assert magnitude < EXACT_BELOW, f"sum |code_x| |code_w| = {magnitude} reaches 2^24: the exact reference does not apply"
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got != want                                           # (+0 == -0; NaN differs from everything)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"H: {int(bad.sum())} of {bad.size} elements differ from the exact sums; first at {i}: "
                             f"got {got[i]!r}, want {want[i]!r}")


def check_D(got, want, bound, names=None):
    R.check("D", np.asarray(got, np.float64), want, bound, np.arange(want.shape[0]), names or {})


def check_layer(got_H, got_D, ref, names=None):
    check_H(got_H, ref["H"], ref["magnitude"])
    check_D(got_D, ref["D"], ref["bound"], names)


# ---- operands whose edges are real ------------------------------------------------------------------------------------

CLIP_SHARE = 5e-4          # at least this share of H on EACH clip bound where the shape can reach it (see operands)


def can_clip(c, k):
    """Can a sum of k products of quantised operands reach the clip bound 2^scale_fea?"""
    b = c.w_qbits
    x_max = (2 ** b - 1) / den(b)
    w_max = 0.5 if b == 1 else (2 ** (b - 1) - 1) / den(b)
    return k * x_max * w_max >= 2 ** c.scale_fea


def features(n, m, c, seed, degs=None, dense=False, hot_every=7):
    """X with values over the whole feature range [0, 1] and past it; every hot_every-th row is 'hot': all its entries
    at the top of the range, so that with the hot columns of weights() its sums pass the clip bound on both signs.
    degs: entries per row of a CSR X (columns drawn with repetition, as the library's CSR allows)."""
    rng = np.random.default_rng([seed, 1])
    if dense:
        X = rng.uniform(-0.1, 1.2, (n, m)).astype(np.float32)
        X[rng.random((n, m)) < 0.3] = 0.0
        X[::hot_every] = 1.1
        return X
    degs = np.asarray(degs, np.int64)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(degs)
    nnz = int(rowptr[-1])
    col = rng.integers(0, m, nnz).astype(np.int32)
    val = rng.uniform(-0.1, 1.2, nnz).astype(np.float32)
    row = np.repeat(np.arange(n), degs)
    val[row % hot_every == 0] = 1.1
    return rowptr.astype(np.int32), col, val


def weights(m, p, c, seed):
    """W [m, p] over the signed weight range and past it; column 0 all at the top of the range, column 1 (if any) all at
    the bottom: a hot row of X sums to +-(its entry count) x_max w_max there."""
    rng = np.random.default_rng([seed, 2])
    w_max = c.w_s * (1 if c.w_qbits == 1 else 2 ** (c.w_qbits - 1) - 1)
    W = (rng.uniform(-1.2, 1.2, (m, p)) * w_max).astype(np.float32)
    W[:, 0] = 1.1 * w_max
    if p > 1:
        W[:, 1] = -1.1 * w_max
    return W


def attention(p, c, seed):
    rng = np.random.default_rng([seed, 3])
    w_max = c.w_s * (1 if c.w_qbits == 1 else 2 ** (c.w_qbits - 1) - 1)
    return (rng.uniform(-1.0, 1.0, 2 * p) * w_max * (0.3 if c.w_qbits > 2 else 1.0)).astype(np.float32)


def adjacency(degs, n_cols, c, seed, zero_share=0.1, dead_rows=()):
    """CSR adjacency with the given entries per row; values over the adjacency range [0, a_max]; zero_share of the
    entries lie below half a quantisation step (stored entries that quantise to exactly 0) and every entry of the rows
    in dead_rows does.  Returns (rowptr, col, val)."""
    rng = np.random.default_rng([seed, 4])
    degs = np.asarray(degs, np.int64)
    n = len(degs)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(degs)
    nnz = int(rowptr[-1])
    col = rng.integers(0, n_cols, nnz).astype(np.int32)
    val = (rng.uniform(0.6, 2 ** c.w_qbits + 0.4, nnz) * c.a_s).astype(np.float32)
    val[rng.random(nnz) < zero_share] = np.float32(0.3 * c.a_s)
    for r in dead_rows:
        val[rowptr[r]:rowptr[r + 1]] = np.float32(0.3 * c.a_s)
    return rowptr.astype(np.int32), col, val


def assert_edges(ref, c, adj=None, a_val=None, clip_terms=None, gat_rows=None):
    """The edges the operands were built for are there, on the reference's own numbers:
    clip_terms: the longest hot row's entry count -- where can_clip() says the bound can be reached, CLIP_SHARE of H
    lies on each clip bound; at 2 and 1 bits the 3-decimal rounding moves values; stored adjacency entries quantise to 0;
    gat_rows = (all_zero_row, empty_row): a row whose every entry quantised to 0 and a row without an entry, both dead."""
    f, H = ref["facts"], ref["H"]
    if clip_terms is not None and can_clip(c, clip_terms) and H.shape[1] > 1:
        assert f["clip_hi"] >= CLIP_SHARE * H.size > 0 and f["clip_lo"] >= CLIP_SHARE * H.size, f
        iq = c.internal_quantization
        a_max = torch.round(torch.tensor((2 ** iq - 1) / 2 ** iq, dtype=torch.float32), decimals=iq - 1).numpy()
        assert (H == a_max).sum() >= f["clip_hi"] and (H == -a_max).sum() >= f["clip_lo"]
    if c.w_qbits <= 2:
        assert f["rounded"] > 0, "the 3-decimal rounding moved nothing"
    if adj is not None:
        aq = ref["aq"]
        assert ((aq == 0) & (np.asarray(a_val) > 0)).sum() > 0 and (aq > 0).sum() > 0
    if gat_rows is not None:
        zero_row, empty_row = gat_rows
        rp = np.asarray(adj[0], np.int64)
        assert rp[zero_row + 1] > rp[zero_row] and not (ref["aq"][rp[zero_row]:rp[zero_row + 1]] > 0).any()
        assert rp[empty_row + 1] == rp[empty_row]
        assert ref["dead"][zero_row] and ref["dead"][empty_row] and not ref["dead"].all()
