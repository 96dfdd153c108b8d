"""The small kernels only the backward and training path runs, each against a plain reference at the sizes where its
loops take another trip: sgx_col_sums, sgx_readout_mean_linear / _backward, sgx_coo_to_csr, sgx_csr_validate,
sgx_relu_mask_backward and sgx_pack_rows.

U = 2^-24 is the unit roundoff of the fp32 sums below; every sum of absolute values is taken in float64.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
GRID_THREADS = 2048 * 256          # util_kernels.hip grid_1d: the grid-stride kernels launch at most this many threads
DTYPES = [torch.float16, torch.float32]
DT_IDS = ["f16", "f32"]


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _host_randn(shape, seed):
    """Normal values from the host generator (the same on every machine), on the device."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to("cuda")


def _padded(t, ld, fill, before=0, after=0):
    """t's values as a view of pitch ld > width into a buffer filled with `fill`: (view, whole buffer [rows, ld])."""
    n, w = t.shape
    buf = torch.full((before + n + after, ld), fill, dtype=torch.float32, device=t.device).to(t.dtype)
    v = buf[before:before + n, :w]
    v.copy_(t)
    return v, buf


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- sgx_col_sums --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("F", [1, 7, 64, 256, 257, 300])
@pytest.mark.parametrize("n", [0, 1, 511, 512, 513, 5003])
def test_col_sums(n, F, dtype):
    """Two fixed-order stages: 512 slabs of ceil(n / 512) rows added row by row, then the 512 slab sums added in order --
    recursive summation, at most ceil(n / 512) + 512 roundings on a column's way: |err| <= (ceil(n / 512) + 512) U sum|x|."""
    from sgracex1_amd import ops
    X = torch.randn((n, F), generator=_gen(n * 1000 + F), device="cuda").to(dtype)
    got = ops.col_sums(X)
    assert got.shape == (F,) and got.dtype == torch.float32
    want = X.double().sum(0)
    bound = (math.ceil(n / 512) + 512) * U * X.double().abs().sum(0)
    err = (got.double() - want).abs()
    print(f"col_sums n={n} F={F} {dtype}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item() if n else 0.0:.3e}")
    assert bool((err <= bound).all())
    if n == 0:
        assert torch.equal(got, torch.zeros(F, device="cuda"))
    assert torch.equal(ops.col_sums(X), got)                               # the order is fixed: the same bits again
    # rows padded with NaN: the pad columns are not read, as a view and as the n_feat < X.shape[1] form
    view, buf = _padded(X, F + 3, NAN)
    assert torch.equal(ops.col_sums(view), got)
    assert torch.equal(ops.col_sums(buf, n_feat=F), got)


# ---- sgx_readout_mean_linear / sgx_readout_mean_backward -----------------------------------------------------------------

SIZES = [0, 17, 1, 0, 300, 5, 0]           # empty graphs first, in the middle and last


def _graph_ptr(first):
    return torch.tensor(np.concatenate([[first], first + np.cumsum(SIZES)]), dtype=torch.int32, device="cuda")


def _readout_case(F, dtype, first):
    """X with `first` rows before the first graph and 2 after the last that belong to no graph and hold NaN."""
    ptr = _graph_ptr(first)
    n = first + sum(SIZES) + 2
    X = _host_randn((n, F), F * 10 + first).to(dtype)
    X[:first] = NAN
    X[first + sum(SIZES):] = NAN
    return X, ptr


def _pool64(X, ptr):
    """float64 means and, per (graph, column), sum |x| / len: the terms of the mean."""
    p = ptr.tolist()
    mean = torch.zeros((len(SIZES), X.shape[1]), dtype=torch.float64, device="cuda")
    mag = torch.zeros_like(mean)
    for g, (a, b) in enumerate(zip(p[:-1], p[1:])):
        if b > a:
            mean[g] = X[a:b].double().sum(0) / (b - a)
            mag[g] = X[a:b].double().abs().sum(0) / (b - a)
    return mean, mag


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("F", [1, 7, 65, 300])
@pytest.mark.parametrize("C", [1, 4, 5, 9])
def test_readout_mean_linear(C, F, dtype):
    """pooled: len additions, the reciprocal and the product: |err| <= (len + 2) U sum|x / len|.
    logits from the fp32 pooled row the kernel holds: per lane ceil(F / 64) fmas, 6 butterfly additions, the bias:
    |err| <= (F / 64 + 8) U sum|w mean|.  With a bias the last addition alone rounds by up to U |logit|, and |logit| is not
    bounded by sum|w mean|, so |bias| joins the sum of the terms' magnitudes there; without a bias the bound stands as it is.
    Observed on these inputs (drawn from the host generator, so the same everywhere), from the float64 reference alone: at
    C = 9, F = 1, fp32, ptr[0] = 4, the graph of 300 rows, class 0, the reference logit is 2.192372884789 = 0.001378622 of
    w mean + 2.190994263 of bias; the nearest fp32 number lies 8.587e-08 from it, while (F / 64 + 8) U sum|w mean| is
    6.59e-10 -- no fp32 result can come closer than 130 times the bound without the bias.  Against the float64 pooling
    the logits carry the pooled rows' own error as well: sum |w| (len + 2) U sum|x / len| more."""
    from sgracex1_amd import ops
    from sgracex1_amd._lib import lib
    W, b = _host_randn((C, F), C * 1000 + F), _host_randn((C,), C * 1000 + F + 500)
    lens = torch.tensor(SIZES, dtype=torch.float64, device="cuda")[:, None]
    for first in (0, 4):
        X, ptr = _readout_case(F, dtype, first)
        mean64, mag = _pool64(X, ptr)
        for bias in (b, None):
            for layout in ("contiguous", "padded"):
                Xv = X if layout == "contiguous" else _padded(X, F + 5, NAN)[0]
                where = f"C={C} F={F} {dtype} ptr[0]={first} bias={bias is not None} {layout}"
                logits, pooled = ops.readout_mean_linear(Xv, ptr, W, bias, want_pooled=True)
                perr, pbound = (pooled.double() - mean64).abs(), (lens + 2) * U * mag
                assert bool((perr <= pbound).all()), where
                terms = (W.double()[None] * pooled.double()[:, None, :]).abs().sum(2)             # [graphs, C]
                lin = pooled.double() @ W.double().t()
                if bias is not None:
                    lin, terms = lin + bias.double(), terms + bias.double().abs()
                lerr, lbound = (logits.double() - lin).abs(), (F / 64 + 8) * U * terms
                bare = (F / 64 + 8) * U * (W.double()[None] * pooled.double()[:, None, :]).abs().sum(2)
                print(f"readout {where}: pooled err/bound {(perr / pbound.clamp_min(1e-300)).max().item():.3e}, "
                      f"logit err/bound {(lerr / lbound.clamp_min(1e-300)).max().item():.3e}, "
                      f"logit err / bound without |bias| {(lerr / bare.clamp_min(1e-300)).max().item():.3e}")
                assert bool((lerr <= lbound).all()), where
                full = mean64 @ W.double().t() + (0 if bias is None else bias.double())
                carried = pbound @ W.double().abs().t()
                assert bool(((logits.double() - full).abs() <= lbound + carried).all()), where
                empty = torch.tensor([s == 0 for s in SIZES], device="cuda")
                assert bool((pooled[empty] == 0).all()), where
                # the same bits from the pooling alone, and logits alone into a buffer that starts as NaN (every class written)
                assert torch.equal(ops.readout_mean_linear(Xv, ptr), pooled), where
                alone = torch.full((len(SIZES), C), NAN, device="cuda")
                rc = lib.sgx_readout_mean_linear(ops.dtype_code(dtype), len(SIZES), F, C, _vp(Xv), Xv.stride(0), _vp(ptr), _vp(W),
                                                 _vp(bias), None, _vp(alone), _stream())
                assert rc == 0 and torch.equal(alone, logits), where


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("F", [1, 7, 65, 300])
def test_readout_mean_backward(F, dtype):
    """include/sgx.h: grad_X[r] = dtype(grad_pooled[g] * (1 / len)), the fp32 reciprocal rounded once, the product rounded
    to fp32 and then to dtype -- restated in numpy and matched bit for bit -- which lies within 2 U (fp32; one rounding to
    fp16 more: 2^-11 and half the smallest subnormal) of grad_pooled / len in float64.  Rows of no graph and pad columns
    are not written."""
    from sgracex1_amd import ops
    from sgracex1_amd._lib import lib
    gp = torch.randn((len(SIZES), F), generator=_gen(F), device="cuda")
    npdt = np.float16 if dtype == torch.float16 else np.float32
    for first in (0, 4):
        ptr = _graph_ptr(first)
        n = first + sum(SIZES) + 2
        p = ptr.tolist()
        want = np.zeros((n, F), dtype=npdt)
        want64 = np.zeros((n, F))
        inside = np.zeros(n, dtype=bool)
        for g, (a, b) in enumerate(zip(p[:-1], p[1:])):
            if b > a:
                row = gp[g].cpu().numpy()
                want[a:b] = (row * (np.float32(1.0) / np.float32(b - a))).astype(npdt)
                want64[a:b] = row.astype(np.float64) / (b - a)
                inside[a:b] = True
        got = ops.readout_mean_backward(gp, ptr, n, dtype)
        assert got.dtype == dtype and got.shape == (n, F)
        assert np.array_equal(got.cpu().numpy(), want)                                     # (rows of no graph: the zeros)
        tol = 2.001 * U * np.abs(want64) + (2.0 ** -11 * np.abs(want64) * (1 + 2.001 * U) + 2.0 ** -25 if dtype == torch.float16 else 0)
        assert (np.abs(got.double().cpu().numpy() - want64) <= tol).all()
        # into a padded buffer of sentinels: only the graphs' rows and the F columns change
        sentinel = -77.0
        buf = torch.full((n, F + 3), sentinel, dtype=dtype, device="cuda")
        rc = lib.sgx_readout_mean_backward(ops.dtype_code(dtype), len(SIZES), F, _vp(gp), _vp(ptr), _vp(buf), F + 3, _stream())
        assert rc == 0
        out = buf.cpu().numpy()
        assert np.array_equal(out[inside, :F], want[inside])
        assert (out[~inside] == sentinel).all() and (out[:, F:] == sentinel).all()


# ---- sgx_coo_to_csr / sgx_csr_validate -----------------------------------------------------------------------------------

def _sorted_rows(nnz, lo, hi, hole, seed):
    """nnz sorted row indices in [lo, hi) with none in hole = [h0, h1)."""
    r = torch.randint(lo, hi - (hole[1] - hole[0]), (nnz,), generator=_gen(seed), device="cuda")
    r = torch.where(r >= hole[0], r + (hole[1] - hole[0]), r)
    return torch.sort(r)[0].to(torch.int32)


def _coo_cases():
    big_rows = 600_011
    return {
        "edges": (1000, lambda: _sorted_rows(5000, 100, 900, (400, 600), 1)),        # empty rows first, last and in a run
        "one_row": (50, lambda: torch.full((3000,), 7, dtype=torch.int32, device="cuda")),
        "last_row": (50, lambda: torch.full((10,), 49, dtype=torch.int32, device="cuda")),
        "nnz0": (10, lambda: torch.zeros(0, dtype=torch.int32, device="cuda")),
        "nothing": (0, lambda: torch.zeros(0, dtype=torch.int32, device="cuda")),
        # more entries (and rows) than the 524 288 threads of the grid: the strided pass
        "strided": (big_rows, lambda: _sorted_rows(600_000, 1000, big_rows - 1000, (300_000, 300_500), 2)),
    }


def _rowptr_ref(row, n_rows):
    want = torch.searchsorted(row.long(), torch.arange(n_rows + 1, device="cuda")).to(torch.int32)    # entries with row < r
    counts = torch.bincount(row.long(), minlength=n_rows) if n_rows else torch.zeros(0, dtype=torch.long, device="cuda")
    assert torch.equal(want[1:].long(), torch.cumsum(counts, 0)) and int(want[0]) == 0
    return want


@pytest.mark.parametrize("case", list(_coo_cases()))
def test_coo_to_csr(case):
    from sgracex1_amd import ops
    from sgracex1_amd._lib import lib
    n_rows, make = _coo_cases()[case]
    row = make()
    if case == "strided":
        assert row.numel() > GRID_THREADS and n_rows > GRID_THREADS
    want = _rowptr_ref(row, n_rows)
    rowptr = torch.full((n_rows + 1,), -7, dtype=torch.int32, device="cuda")
    assert lib.sgx_coo_to_csr(_vp(row), row.numel(), n_rows, _vp(rowptr), _stream()) == 0
    assert torch.equal(rowptr, want)
    if row.numel():
        col = torch.zeros_like(row)
        A = ops.Csr.from_coo(row, col, torch.ones(row.numel(), dtype=torch.float16, device="cuda"), n_rows, 3)
        assert torch.equal(A.rowptr, want)
        A.validate()


def test_csr_validate_each_defect():
    """Every defect alone, once at index 0 and once past the grid's 524 288 threads (the strided pass of each loop)."""
    from sgracex1_amd import ops
    from sgracex1_amd._lib import SgxError
    n_rows, make = _coo_cases()["strided"]
    n_cols = 1000
    row = make()
    nnz = row.numel()
    rowptr = _rowptr_ref(row, n_rows)
    col = torch.randint(0, n_cols, (nnz,), generator=_gen(3), device="cuda").to(torch.int32)
    col[0], col[nnz - 1] = 0, n_cols - 1                               # the extremes that are still valid
    val = torch.ones(nnz, dtype=torch.float16, device="cuda")
    ops.Csr(rowptr, col, val, n_cols).validate()
    far_row, far_e = GRID_THREADS + 30_001, GRID_THREADS + 50_001
    assert far_row + 2 < n_rows and far_e < nnz and int(rowptr[1]) == 0

    def broken(what, at):
        rp, c = rowptr.clone(), col.clone()
        if what == "first":
            rp[0] = -1                                                 # (not a decreasing pair: rowptr[1] = 0)
        elif what == "last":
            rp[n_rows] = nnz + 1
        elif what == "decreasing":
            rp[at + 1] = rp[at] - 1                                    # rowptr[at + 2] >= rowptr[at]: one pair only
        elif what == "negative":
            c[at] = -1
        elif what == "too_large":
            c[at] = n_cols
        return ops.Csr(rp, c, val, n_cols)

    for what, places in [("first", [0]), ("last", [0]), ("decreasing", [0, far_row]), ("negative", [0, far_e]),
                         ("too_large", [0, far_e])]:
        for at in places:
            with pytest.raises(SgxError) as e:
                broken(what, at).validate()
            assert e.value.status == -6, (what, at)                    # SGX_ERR_CSR


# ---- sgx_relu_mask_backward ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gdtype", DTYPES, ids=["grad_f16", "grad_f32"])
@pytest.mark.parametrize("odtype", DTYPES, ids=["out_f16", "out_f32"])
def test_relu_mask_backward(odtype, gdtype):
    from sgracex1_amd import ops
    n = 600_001                                                        # over the grid's 524 288 threads, and ragged
    assert n > GRID_THREADS
    g = _gen(11)
    palette = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, -1.5, -65504.0, NAN, 1.0, 0.33], device="cuda").to(odtype)
    out = palette[torch.randint(0, palette.numel(), (n,), generator=g, device="cuda")]
    out[0], out[n - 1], out[GRID_THREADS] = 0.0, -0.0, 0.0            # the ends and the first element of the second pass
    assert bool((out == 2.0 ** -24).any()) and bool(out.isnan().any())         # the smallest fp16 subnormal survives the cast
    grad = torch.randn(n, generator=g, device="cuda").to(gdtype)
    grad[5::97] = NAN
    before = grad.clone()
    res = ops.relu_mask_backward_(out, grad)
    assert res is grad
    zero = out == 0                                                    # +0 and -0; not NaN, not a subnormal
    assert 0.15 < zero.float().mean().item() < 0.3
    assert bool((_bits(grad)[zero] == 0).all())                       # exactly +0
    assert torch.equal(_bits(grad)[~zero], _bits(before)[~zero])     # kept bit for bit, also where out is NaN
    assert bool(grad[out.isnan() & ~before.isnan()].isfinite().all())


# ---- sgx_pack_rows -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("F", [1, 3, 7, 8, 9, 64, 300])
def test_pack_rows(F, dtype):
    """16-byte chunks with a tail of row_bytes % 16 bytes copied two at a time: whole chunks only (F = 8, 64), a tail only
    (F = 1, 3, 7 in fp16; 1, 3 in fp32), both (the rest)."""
    from sgracex1_amd import ops
    g = _gen(F)
    n_src = 300
    src = torch.randn((n_src, F), generator=g, device="cuda").to(dtype)
    idx = torch.randint(0, n_src, (1000,), generator=g, device="cuda").to(torch.int32)       # out of order, with repeats
    idx[:4] = torch.tensor([n_src - 1, 0, 0, n_src - 1], dtype=torch.int32)
    assert idx.unique().numel() < idx.numel() and bool((idx[1:] < idx[:-1]).any())
    want = src.index_select(0, idx.long())
    assert torch.equal(_bits(ops.pack_rows(src, idx)), _bits(want))
    # a padded source whose pads hold NaN, into a padded destination of sentinels
    sv = _padded(src, F + 3, NAN, before=2, after=2)[0]
    sentinel = -3.0
    buf = torch.full((idx.numel(), F + 5), sentinel, dtype=dtype, device="cuda")
    res = ops.pack_rows(sv, idx, out=buf[:, :F])
    assert res.data_ptr() == buf.data_ptr()
    assert torch.equal(_bits(buf[:, :F].contiguous()), _bits(want))
    assert bool((buf[:, F:] == sentinel).all())
    # no rows
    none = ops.pack_rows(src, idx[:0])
    assert none.shape == (0, F)
    keep = buf.clone()
    ops.pack_rows(sv, idx[:0], out=buf[:0, :F])
    assert torch.equal(_bits(buf), _bits(keep))


def test_pack_rows_strided_pass():
    """More 16-byte chunks than the grid's 8192 x 256 threads: every lane copies a second chunk."""
    from sgracex1_amd import ops
    g = _gen(5)
    src = torch.randn((1000, 8), generator=g, device="cuda").half()
    idx = torch.randint(0, 1000, (8192 * 256 + 1001,), generator=g, device="cuda").to(torch.int32)
    assert torch.equal(ops.pack_rows(src, idx), src.index_select(0, idx.long()))
