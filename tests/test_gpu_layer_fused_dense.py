"""The fused form of a square dense fp16 layer (64 -> 64): the aggregation of X with W applied in its epilogue, one launch,
D = act(f16(A.X) . W) with neither H nor Z in memory (spmm_dense_f16_kernel, csrc/spmm_csr.hip; fused_dense_form,
csrc/layer.hip).

References, neither of them the code under test: the staged forms ops.spmm and ops.xw_dense (the ReLU as in
test_aggregate_first_order), to which the fused layer is BIT-EQUAL under both orders, and numpy float64 on the same fp16
inputs at the fp16 tolerance of test_layer_forward_random_case (rtol 1e-2, atol 3e-3).  Whether a call takes the fused
form is read from sgx_layer_workspace_bytes: the fused form needs no workspace, every staged form does."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = 64
TOL = dict(rtol=1e-2, atol=3e-3)
NO_FUSED = dict(SGX_LAYER_NO_FUSED_DENSE="1")


def _csr(n_rows, n_cols, seed, empty=(), long_row=None, dtype=torch.float16):
    """Rows of 17 .. 24 entries (three 8-entry steps each, so a plan keeps the natural order), `empty` rows without any,
    `long_row` = (row, entries)."""
    from sgracex1_amd import ops
    rng = np.random.default_rng(seed)
    deg = rng.integers(17, 25, n_rows)
    deg[list(empty)] = 0
    if long_row is not None:
        deg[long_row[0]] = long_row[1]
    rp = np.zeros(n_rows + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    col = rng.integers(0, n_cols, rp[-1]).astype(np.int32)
    val = (rng.random(rp[-1]) * 0.08 + 0.02).astype(np.float32)
    return ops.Csr(torch.as_tensor(rp, device="cuda"), torch.as_tensor(col, device="cuda"),
                   torch.as_tensor(val, device="cuda").to(dtype), n_cols)


def _operands(n_cols, seed, P=F, dtype=torch.float16):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    X = (torch.rand((n_cols, F), generator=g, device="cuda") - 0.3).to(dtype)
    Wt = ((torch.rand((P, F), generator=g, device="cuda") * 2 - 1) / 8).to(dtype)
    return X, Wt


def _desc(A, X, Wt, out, use_plan=True, order=0, acc_mode=0):
    from sgracex1_amd import _lib, ops
    d = _lib.LayerDesc()
    d.gemm_mode, d.dtype, d.acc_mode, d.order, d.spmm_block = 1, ops.dtype_code(Wt.dtype), acc_mode, order, 1
    d.N_adj, d.M_adj, d.M_fea, d.P_w = A.n_rows, A.n_cols, Wt.shape[1], Wt.shape[0]
    d.rowPtr_adj, d.columnIndex_adj, d.values_adj = A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr()
    d.values_fea, d.B, d.D = X.data_ptr(), Wt.data_ptr(), out.data_ptr()
    if use_plan and A.wants_plan:
        d.plan_adj = A.plan.handle
    return d


def _workspace_bytes(A, X, Wt, **kw):
    from sgracex1_amd import _lib
    out = torch.empty((A.n_rows, Wt.shape[0]), dtype=Wt.dtype, device="cuda")
    return _lib.lib.sgx_layer_workspace_bytes(ctypes.byref(_desc(A, X, Wt, out, **kw)))


def _staged(A, X, Wt, relu, use_plan=True):
    from sgracex1_amd import ops
    H = ops.xw_dense(ops.spmm(A, X, use_plan=use_plan), Wt)
    return torch.where(H > 0, H, torch.zeros_like(H)) if relu else H


def _f64(A, X, Wt, relu):
    rp = A.rowptr.cpu().numpy()
    col, val = A.col.cpu().numpy()[:rp[-1]], A.val.cpu().numpy().astype(np.float64)[:rp[-1]]
    Z = np.zeros((A.n_rows, X.shape[1]))
    np.add.at(Z, np.repeat(np.arange(A.n_rows), np.diff(rp)), val[:, None] * X.cpu().numpy().astype(np.float64)[col])
    D = Z @ Wt.cpu().numpy().astype(np.float64).T
    return np.maximum(D, 0) if relu else D


def _check_fused(A, X, Wt, use_plan=True):
    """Both orders, ReLU on and off: the fused form is taken, equals the staged launches bit for bit and float64 within
    the fp16 tolerance; rows without entries are exactly +0."""
    from sgracex1_amd import ops
    assert _workspace_bytes(A, X, Wt, use_plan=use_plan) == 0 and _workspace_bytes(A, X, Wt, use_plan=use_plan, order=1) == 0
    empty = torch.as_tensor(np.diff(A.rowptr.cpu().numpy()) == 0, device="cuda")
    for relu in (False, True):
        staged, want = _staged(A, X, Wt, relu, use_plan), _f64(A, X, Wt, relu)
        for order in ("reference", "aggregate_first"):
            got = ops.layer_forward(A, X, Wt, relu=relu, order=order, use_plan=use_plan)
            assert got.shape == (A.n_rows, F) and torch.equal(got, staged), (relu, order)
            np.testing.assert_allclose(got.float().cpu().numpy(), want, **TOL)
            # +0, not -0: all sixteen bits clear
            assert not got[empty].view(torch.int16).any()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 4099])
def test_fused_layer_equals_the_staged_launches(n):
    """Every tail of the 8-row group, the 16-row tile and the workgroup's 64 rows; 4099 rows: a plan (no row cut, natural
    order) and more than one workgroup."""
    A = _csr(n, n, seed=n)
    if n == 4099:
        assert A.wants_plan and not A.plan.reordered and A.plan.long_rows == 0
    X, Wt = _operands(n, seed=n + 1)
    _check_fused(A, X, Wt)


def test_rectangular_adjacency_and_rows_without_entries():
    """N_adj != M_adj, and empty rows at the start, middle and end of a 16-row tile and of the matrix."""
    n, m = 1043, 2500                                 # 1043 = 65 tiles + 3 rows
    empty = (0, 7, 8, 15, 16, 23, 31, 520, 521, 1024, 1039, 1040, 1042)
    A = _csr(n, m, seed=5, empty=empty)
    assert A.wants_plan and not A.plan.reordered and A.plan.long_rows == 0
    X, Wt = _operands(m, seed=6)
    _check_fused(A, X, Wt)
    # a whole tile and a whole workgroup of empty rows
    A2 = _csr(300, m, seed=7, empty=tuple(range(64, 128)) + tuple(range(144, 160)))
    _check_fused(A2, X, Wt)


def test_graph_given_without_a_plan():
    A = _csr(4099, 4099, seed=11)
    X, Wt = _operands(4099, seed=12)
    assert A.wants_plan
    _check_fused(A, X, Wt, use_plan=False)


def _assert_old_path(A, X, Wt, **kw):
    """Not the fused form: the workspace and the bits of the call under SGX_LAYER_NO_FUSED_DENSE."""
    from sgracex1_amd import _lib, ops
    desc_kw = {k: v for k, v in kw.items() if k == "acc_mode"}
    got = ops.layer_forward(A, X, Wt, relu=True, **kw)
    nbytes = _workspace_bytes(A, X, Wt, **desc_kw)
    with _lib.tuning(**NO_FUSED):
        assert _workspace_bytes(A, X, Wt, **desc_kw) == nbytes > 0
        assert torch.equal(ops.layer_forward(A, X, Wt, relu=True, **kw), got)
    return got


def test_fallbacks_take_the_old_path_and_its_bits():
    from sgracex1_amd import graphs, ops
    n = 3000
    X, Wt = _operands(n, seed=21)
    # one row longer than the plan's cut: the plan holds tasks
    A = _csr(n, n, seed=22, long_row=(1500, 700))
    assert A.plan.long_rows == 1 and 700 > A.plan.long_threshold
    got = _assert_old_path(A, X, Wt)
    np.testing.assert_allclose(got.float().cpu().numpy(), _f64(A, X, Wt, True), **TOL)
    # a power-law graph whose plan lists the rows in degree order
    R = graphs.rmat_graph(12, 60_000, seed=23)
    assert R.plan.reordered
    Xr, _ = _operands(R.n_cols, seed=24)
    _assert_old_path(R, Xr, Wt)
    # not square, not fp16, not the default arithmetic
    U = _csr(n, n, seed=25)
    _assert_old_path(U, X, _operands(n, seed=26, P=47)[1])
    X32, Wt32 = _operands(n, seed=27, dtype=torch.float32)
    _assert_old_path(_csr(n, n, seed=25, dtype=torch.float32), X32, Wt32)
    _assert_old_path(U, X, Wt, acc_mode=ops.SGX_ACC_REF_HALF)
    # (ops hands the layer a dense X at pitch M_fea only: there is no padded view to pass)
    with pytest.raises(ValueError):
        ops.layer_forward(U, torch.empty((n, 72), dtype=torch.float16, device="cuda")[:, :F], Wt)


def test_the_override_gives_the_staged_reference_order():
    """With SGX_LAYER_NO_FUSED_DENSE the default order is X.W first again: A.(X.W), its own bits."""
    from sgracex1_amd import _lib, ops
    A = _csr(2000, 2000, seed=31)
    X, Wt = _operands(2000, seed=32)
    with _lib.tuning(**NO_FUSED):
        old = ops.layer_forward(A, X, Wt, relu=True)
        assert torch.equal(old, ops.spmm(A, ops.xw_dense(X, Wt), relu=True))
        assert torch.equal(ops.layer_forward(A, X, Wt, relu=True, order="aggregate_first"), _staged(A, X, Wt, True))
    np.testing.assert_allclose(old.float().cpu().numpy(), _f64(A, X, Wt, True), **TOL)


@pytest.mark.parametrize("offset", [64, 24, 3])
def test_no_stray_writes(offset):
    """`out` is a slice of a larger buffer filled with NaN, on a line, on 16 bytes and on an odd half: the halves before and
    after it keep their bits, for a row count that ends inside a tile."""
    from sgracex1_amd import ops
    n = 1043
    A = _csr(n, n, seed=41)
    X, Wt = _operands(n, seed=42)
    buf = torch.full((offset + n * F + 256,), float("nan"), dtype=torch.float16, device="cuda")
    before = buf.view(torch.int16).clone()
    out = buf[offset:offset + n * F].view(n, F)
    ops.layer_forward(A, X, Wt, relu=False, out=out)
    assert torch.equal(out, _staged(A, X, Wt, False))
    after = buf.view(torch.int16)
    assert torch.equal(after[:offset], before[:offset]) and torch.equal(after[offset + n * F:], before[offset + n * F:])


def test_replayed_from_a_hipgraph():
    from sgracex1_amd import ops
    from sgracex1_amd.graphed import Graphed
    n = 4099
    A = _csr(n, n, seed=51)
    X, Wt = _operands(n, seed=52)
    out = torch.empty((n, F), dtype=torch.float16, device="cuda")
    run = Graphed(lambda: ops.layer_forward(A, X, Wt, relu=True, out=out))
    X.mul_(-0.5)
    out.zero_()
    run()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.layer_forward(A, X, Wt, relu=True)) and torch.equal(out, _staged(A, X, Wt, True))
    assert out.abs().max() > 0


def test_workspace_of_the_fused_form():
    """Smaller than the staged form's, and a call given exactly that many bytes -- none -- succeeds."""
    from sgracex1_amd import _lib
    n = 2000
    A = _csr(n, n, seed=61)
    X, Wt = _operands(n, seed=62)
    out = torch.empty((n, F), dtype=torch.float16, device="cuda")
    for order in (0, 1):
        d = _desc(A, X, Wt, out, order=order)
        d.relu = 1
        fused_bytes = _lib.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
        with _lib.tuning(**NO_FUSED):
            assert fused_bytes < _lib.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
        assert fused_bytes == 0
        d.workspace, d.workspace_bytes = None, 0
        out.fill_(float("nan"))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib.sgx_layer_forward(ctypes.byref(d), stream), "sgx_layer_forward")
        torch.cuda.synchronize()
        assert torch.equal(out, _staged(A, X, Wt, True))
