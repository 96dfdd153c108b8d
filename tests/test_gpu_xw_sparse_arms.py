"""Every arm of the sparse X.W stage's LDS form (csrc/xw_sparse_lds.hip) against float64, on the deterministic inputs of
tests/_xw_sparse_ref.py (built around the kernel's windows of 64 rows, sub-tiles of 64 / LPR rows and units of 8 steps).

Every case first asserts WHICH kernel runs: ops.xw_sparse_form (sgx_xw_sparse_form, answered by the functions the launch
uses) names the intended arm -- lanes per row, slices, 16-byte or element stores, 16-byte or element fills of W's slice,
streams of the grid -- and under SGX_XW_SPARSE_NO_LDS the same call names the gather kernel.  Then:
  (a) every element within (n + 2) 2^-24 (|X| @ |W|) plus one store rounding of the float64 sum (derived in
      _spmm_acc_ref.py; tests/test_xw_sparse_ref_cpu.py shows one entry lost or gained, rows or slices misplaced and a
      skipped unit land outside it in every row they touch);
  (b) the same bits as the gather kernel (the same call under SGX_XW_SPARSE_NO_LDS: the same fp32 fma chain per element);
  (c) rows without an entry exactly +0."""
import functools

import numpy as np
import pytest
import torch

import _spmm_acc_ref as R
import _xw_sparse_ref as X

pytestmark = pytest.mark.gpu
TDT = {"f16": torch.float16, "f32": torch.float32}
BITS = {"f16": torch.int16, "f32": torch.int32}
SENTINEL = -77.0


@functools.lru_cache(maxsize=None)
def csr(name, dt):
    from sgracex1_amd import ops
    rp, ci, va = X.matrix(name, dt)
    M = ops.Csr(torch.as_tensor(rp, device="cuda"), torch.as_tensor(ci, device="cuda"), torch.as_tensor(va).to(TDT[dt]).cuda(),
                X.n_cols(name))
    assert M.nnz >= 1 << 20 and M.plan.long_threshold == X.PLAN_CUT and M.plan.long_rows == 0
    return M


def table(name, P, dt, pitch=None, fill=float("nan")):
    """W on the device; pitch: a column view of rows of that many elements, the columns beyond P filled with `fill`"""
    W = torch.as_tensor(X.weights(name, P, dt)).to(TDT[dt]).cuda()
    if pitch is None:
        return W.contiguous()
    buf = torch.full((W.shape[0], pitch), fill, dtype=TDT[dt], device="cuda")
    buf[:, :P] = W
    return buf[:, :P]


def _np(t):
    return t.double().cpu().numpy()


def _bits(t, dt):
    return t.contiguous().view(BITS[dt])


def expected_arm(name, dt, W, out=None, **kw):
    """the restated selection for the operands as they are passed"""
    Xm = csr(name, dt)
    P = W.shape[1]
    return X.arm(dt, Xm.n_rows, Xm.n_cols, P, Xm.nnz, X.PLAN_CUT if name != "wide" else 200,
                 w_aligned=W.data_ptr() % 16 == 0, ldw=W.stride(0),
                 h_aligned=out is None or out.data_ptr() % 16 == 0, ldh=P if out is None else out.stride(0), **kw)


def run(name, dt, W, want_arm, tune=None, make_out=None):
    """The LDS form's result for fixture `name`, after asserting that it is the arm `want_arm` (lpr, n_split, full and, where
    given, the other fields) that runs, and that the gather kernel's result has the same bits.  make_out: builds `out`
    (a fresh one per kernel).  Returns (result, form)."""
    from sgracex1_amd import _lib, ops
    Xm = csr(name, dt)
    tune = dict(tune or {})
    out = make_out() if make_out else None
    with _lib.tuning(**tune):
        form = ops.xw_sparse_form(Xm, W, out=out)
        assert form is not None, "the gather kernel would run"
        assert form._asdict() == {**form._asdict(), **want_arm}, (form, want_arm)
        restated = expected_arm(name, dt, W, out, lpr_cap=int(tune.get("SGX_XW_SPARSE_LPR") or 0),
                                streams_cap=int(tune.get("SGX_XW_SPARSE_STREAMS") or 0))
        assert tuple(form) == tuple(restated), (form, restated)
        got = ops.xw_sparse(Xm, W, out=out)
    out2 = make_out() if make_out else None
    with _lib.tuning(**{**tune, "SGX_XW_SPARSE_NO_LDS": "1"}):
        assert ops.xw_sparse_form(Xm, W, out=out2) is None
        gathered = ops.xw_sparse(Xm, W, out=out2)
    assert torch.equal(_bits(got, dt), _bits(gathered, dt)), "LDS form and gather kernel differ"
    return got, form


def check(name, dt, P, got):
    """(a) and (c) of the module docstring"""
    want, bound, n = X.reference(name, dt, P)
    assert got.dtype == TDT[dt] and tuple(got.shape) == want.shape
    R.assert_within(f"{name} {dt} P={P}", _np(got), want, bound)
    empty = torch.as_tensor(n == 0, device="cuda")
    assert int(empty.sum()) >= 64 and not _bits(got, dt)[empty].any()         # +0, not -0


@pytest.mark.parametrize("dt,P,cap,lpr,n_split,full", X.DEEP_CASES)
def test_lane_splits_and_slices(dt, P, cap, lpr, n_split, full):
    """`deep`: every lane split (the natural one of the shape, the narrower ones through SGX_XW_SPARSE_LPR), one to four
    slices with the last one full and ragged, 16-byte and element stores -- over windows without an entry, a row at the
    plan's cut, rows of exactly one, two, three units and one entry more or less, all-empty last sub-tiles, an odd entry
    count and an empty row before the last"""
    W = table("deep", P, dt)
    got, form = run("deep", dt, W, dict(lpr=lpr, n_split=n_split, full=full, streams=8),
                    tune={"SGX_XW_SPARSE_LPR": cap, "SGX_XW_SPARSE_STREAMS": None})
    check("deep", dt, P, got)


def test_lane_split_table_covers_every_arm():
    seen = {(dt, lpr, full, n_split) for dt, _, _, lpr, n_split, full in X.DEEP_CASES}
    assert {k[:3] for k in seen} == {(dt, lpr, full) for dt in TDT for lpr in (2, 4, 8, 16) for full in (True, False)}
    assert {k[3] for k in seen} == {1, 2, 3, 4}


# (dtype, P, pitch in elements or None, w_vec, lpr): a column view whose pitch is a multiple of 16 bytes (a ragged last slice
# reads NaN padding into lanes it never stores); pitches that are multiples of 4 but not of 16 bytes; fp16 rows on odd halves
W_LAYOUTS = [
    ("f16", 64, None, True, 8), ("f16", 24, 40, True, 4), ("f16", 100, 104, True, 16), ("f16", 64, 66, False, 8),
    ("f16", 47, None, False, 8), ("f16", 21, None, False, 4),
    ("f32", 64, None, True, 16), ("f32", 21, 24, True, 8), ("f32", 64, 65, False, 16), ("f32", 41, 43, False, 16),
]


@pytest.mark.parametrize("dt,P,pitch,w_vec,lpr", W_LAYOUTS)
def test_w_layouts(dt, P, pitch, w_vec, lpr):
    from sgracex1_amd import ops
    W = table("deep", P, dt, pitch)
    assert ops._gatherable(W, P, csr("deep", dt).nnz) is W              # passed on as it is, not copied
    assert W.stride(0) == (pitch or P) and (W.stride(0) * W.element_size() % 16 == 0) == w_vec
    if (dt, pitch) == ("f16", None) and P % 2:
        assert W.shape[0] * P < 1 << 16 and W.stride(0) * 2 % 4 == 2    # rows on odd halves
    got, form = run("deep", dt, W, dict(lpr=lpr, w_vec=w_vec))
    assert torch.isfinite(got).all()                                    # the NaN padding reached no stored sum
    check("deep", dt, P, got)


# (dtype, P, columns left of H, pitch, full): aligned views with a 16-byte pitch; a pitch that is not one; a base
# off by one element; a ragged P in an aligned view
H_LAYOUTS = [
    ("f16", 64, 8, 80, True), ("f16", 64, 8, 82, False), ("f16", 64, 1, 80, False), ("f16", 47, 8, 64, False),
    ("f16", 16, 8, 32, True), ("f16", 16, 3, 32, False),
    ("f32", 64, 4, 72, True), ("f32", 64, 4, 73, False), ("f32", 64, 1, 72, False), ("f32", 41, 4, 48, False),
    ("f32", 8, 4, 16, True), ("f32", 8, 4, 15, False),
]


@pytest.mark.parametrize("dt,P,left,pitch,full", H_LAYOUTS)
def test_h_layouts(dt, P, left, pitch, full):
    """out= a column view of a buffer filled with a sentinel: the columns on both sides and 3 guard rows before and behind
    keep it, bit for bit"""
    n = csr("deep", dt).n_rows
    bufs = []

    def make_out():
        buf = torch.full((n + 6, pitch), SENTINEL, dtype=TDT[dt], device="cuda")
        bufs.append(buf)
        return buf[3:3 + n, left:left + P]

    W = table("deep", P, dt)
    got, form = run("deep", dt, W, dict(full=full), make_out=make_out)
    assert got.data_ptr() == bufs[0][3:, left:].data_ptr() and got.stride(0) == pitch
    aligned = got.data_ptr() % 16 == 0 and pitch * got.element_size() % 16 == 0
    assert full == (aligned and P % (form.lpr * X.per16(dt)) == 0)
    for buf in bufs:                                                    # the LDS form's buffer, then the gather kernel's
        assert (buf[:3] == SENTINEL).all() and (buf[3 + n:] == SENTINEL).all()
        assert (buf[:, :left] == SENTINEL).all() and (buf[:, left + P:] == SENTINEL).all()
    check("deep", dt, P, got)


@pytest.mark.parametrize("dt,P,lpr,n_split,full", X.WIDE_CASES)
def test_window_walk(dt, P, lpr, n_split, full):
    """`wide` (389 windows) under SGX_XW_SPARSE_STREAMS = 8, 16 and unset: at 8 streams every wavefront walks 3 windows and
    the first five walk 4 -- the rotation of the prefetched order and row pointers across windows; the three runs have
    the same bits and are within the bound"""
    n_rows = csr("wide", dt).n_rows
    W = table("wide", P, dt)
    outs = {}
    for cap, streams in ((8, 8), (16, 16), (None, 32)):
        got, form = run("wide", dt, W, dict(lpr=lpr, n_split=n_split, full=full, streams=streams),
                        tune={"SGX_XW_SPARSE_STREAMS": cap})
        walked = X.windows_per_wavefront(n_rows, form.streams)
        assert walked == {8: [4] * 5 + [3] * 123, 16: [2] * 133 + [1] * 123, 32: [1] * 389 + [0] * 123}[streams]
        outs[streams] = got
    assert torch.equal(_bits(outs[8], dt), _bits(outs[32], dt)) and torch.equal(_bits(outs[16], dt), _bits(outs[32], dt))
    check("wide", dt, P, outs[8])


@pytest.mark.parametrize("dt,P,lpr", X.HOSTILE_CASES)
def test_hostile_neighbours(dt, P, lpr):
    """`hostile`: the first entry of six short rows is +inf, -inf, NaN or refers to a row of W that is; the CSR row before each
    has 1, 3 or 5 entries, so its last step's spare slots HOLD that entry: without the select of the value, or of the
    column, the row before turns NaN.  The non-finite elements are those of float64, element by element."""
    W = table("hostile", P, dt)
    got, form = run("hostile", dt, W, dict(lpr=lpr))
    want, bound, n = X.reference("hostile", dt, P)
    g = _np(got)
    chosen, before = X.hostile_rows()
    for kind in (np.isnan, np.isposinf, np.isneginf):
        wrong = np.nonzero((kind(g) != kind(want)).any(1))[0]
        assert wrong.size == 0, (f"{kind.__name__} differs from float64 in rows {wrong[:8].tolist()}; chosen rows {chosen}, the rows "
                                 f"before them (poisoned by a missing select) {before}: {sorted(set(wrong) & set(before))} among them")
    fin = np.isfinite(want)
    assert (~fin).any(1).sum() == len(chosen)
    R.assert_within(f"hostile {dt} P={P}", np.where(fin, g, 0.0), np.where(fin, want, 0.0), bound)
    empty = torch.as_tensor(n == 0, device="cuda")
    assert int(empty.sum()) >= 64 and not _bits(got, dt)[empty].any()


@pytest.mark.parametrize("dt,P,lpr", [("f16", 64, 8), ("f32", 64, 16)])
def test_inside_the_layer(dt, P, lpr):
    """sgx_layer_forward over `deep` with an identity adjacency: its first stage writes H at the library's own pitch, which at
    these widths is P (the form is the one of the packed call); act(H) within the bound, and equal to the stages run one by one"""
    from sgracex1_amd import ops
    Xm = csr("deep", dt)
    n = Xm.n_rows
    W = table("deep", P, dt)
    assert ops.table_pitch(P, W.element_size()) == P
    form = ops.xw_sparse_form(Xm, W)
    assert form is not None and (form.lpr, form.n_split, form.full) == (lpr, 1, True)
    eye = ops.Csr(torch.arange(n + 1, dtype=torch.int32, device="cuda"), torch.arange(n, dtype=torch.int32, device="cuda"),
                  torch.ones(n, dtype=TDT[dt], device="cuda"), n)
    Wt = W.t().contiguous()
    got = ops.layer_forward(eye, Xm, Wt, relu=True)
    s, scale, n_terms = X.sums("deep", dt, P)
    R.assert_within(f"layer {dt}", _np(got), *R.finished(s, R.partial_bound(n_terms, scale), dt, relu=True))
    H = ops.spmm(Xm, ops.transpose(Wt), relu=False)
    assert torch.equal(got, torch.where(H > 0, H, torch.zeros_like(H)))
