"""The entry-split schedules of the one-call backward, as far as they go without a GPU: the new symbols and descriptor fields,
every argument error of sgx_gat_attention_grad_flat and of sgx_layer_backward's new fields on made-up addresses (nothing
reaches a device: the checks come first), the workspace layout's sizes, sgx_layer_backward_schedule on all 8 combinations,
and the numpy emulation of the attention-gradient rule (tests/_attention_grad_flat_ref.py) against float64 at T = 256, 128."""
import ctypes

import numpy as np
import pytest

import _attention_grad_flat_ref as R

ADDR = 0x10000            # a made-up, 256-byte aligned device address: never dereferenced by the checks
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import _lib
    return _lib


def test_symbols_and_fields(L):
    for name in ("sgx_gat_attention_grad_flat", "sgx_gat_attention_grad_flat_workspace_bytes", "sgx_layer_backward_schedule"):
        assert name in L.SYMBOLS and hasattr(L.lib, name)
    fields = dict(L.LayerGradDesc._fields_)
    assert [fields[k] for k in ("schedule_adj", "schedule_fea", "schedule_xt")] == [ctypes.c_int32] * 3
    assert fields["nnz_fea"] is ctypes.c_int64 and fields["nnz_xt"] is ctypes.c_int64
    names = [f for f, _ in L.LayerGradDesc._fields_]
    assert names[-5:] == ["schedule_adj", "schedule_fea", "schedule_xt", "nnz_fea", "nnz_xt"]       # appended behind the old ones
    d = L.LayerGradDesc()
    assert (d.schedule_adj, d.schedule_fea, d.schedule_xt, d.nnz_fea, d.nnz_xt) == (0, 0, 0, 0, 0)


# ---- sgx_gat_attention_grad_flat ------------------------------------------------------------------------------------------

def _ag(L, **over):
    a = dict(n_rows=10, n_cols=12, n_feat=8, nnz=100, rowPtr=ADDR, columnIndex=ADDR, sg=ADDR, g1=ADDR, Wh=ADDR, ldw=8,
             grad_attention=ADDR, workspace=ADDR, workspace_bytes=1 << 20)
    a.update(over)
    return L.lib.sgx_gat_attention_grad_flat(a["n_rows"], a["n_cols"], a["n_feat"], a["nnz"], a["rowPtr"], a["columnIndex"], a["sg"],
                                             a["g1"], a["Wh"], a["ldw"], a["grad_attention"], a["workspace"], a["workspace_bytes"], None)


def test_attention_grad_flat_argument_errors(L):
    need = L.lib.sgx_gat_attention_grad_flat_workspace_bytes(100, 10, 8)
    assert need > 0 and need % 256 == 0
    for over in (dict(n_rows=-1), dict(n_cols=9), dict(n_feat=0), dict(ldw=7), dict(nnz=-1), dict(nnz=INT32_MAX + 1)):
        assert _ag(L, **over) == L.SGX_ERR_SHAPE, over
    for name in ("grad_attention", "rowPtr", "columnIndex", "sg", "g1", "Wh"):
        assert _ag(L, **{name: None}) == L.SGX_ERR_NULL, name
    assert _ag(L, n_rows=0, n_cols=0, grad_attention=None) == L.SGX_ERR_NULL
    assert _ag(L, n_cols=1 << 30, ldw=8) == L.SGX_ERR_UNSUPPORTED                      # Wh past 32-bit byte offsets
    assert _ag(L, workspace=None) == L.SGX_ERR_WORKSPACE
    assert _ag(L, workspace_bytes=need - 1) == L.SGX_ERR_WORKSPACE
    assert _ag(L, workspace=ADDR + 16) == L.SGX_ERR_ALIGN
    for bad in ((-1, 10, 8), (INT32_MAX + 1, 10, 8), (100, -1, 8), (100, 10, 0)):
        assert L.lib.sgx_gat_attention_grad_flat_workspace_bytes(*bad) == 0, bad


def test_attention_grad_flat_workspace_follows_the_rule(L):
    T = L.lib.sgx_spmm_flat_chunk()
    size = L.lib.sgx_gat_attention_grad_flat_workspace_bytes
    for nnz, n, F in ((0, 0, 1), (1, 1, 3), (T, T, 8), (T + 1, T + 1, 100), (3 * T + 5, 2 * T + 3, 256), (INT32_MAX, 5, 4)):
        units = max(1, -(-nnz // T)) + -(-n // T)
        want = -(-(units * (-(-F // 4) * 4) * 4) // 256) * 256
        assert size(nnz, n, F) == want, (nnz, n, F)


# ---- sgx_layer_backward's descriptor ---------------------------------------------------------------------------------------

def _desc(L, gat=1, gemm=0, **over):
    d = L.LayerGradDesc()
    d.gat_mode, d.gemm_mode, d.N_adj, d.M_adj, d.M_fea, d.P_w = gat, gemm, 300, 300, 20, 64
    d.dtype_adj, d.dtype_x, d.gat_heads, d.alpha, d.nnz_adj = L.SGX_F32, L.SGX_F32, 1, 0.2, 2000
    for name in ("rowPtr_adj", "columnIndex_adj", "values_adj", "W", "G", "grad_weights", "grad_attention", "grad_input", "E", "S"):
        setattr(d, name, ADDR)
    d.ldg, d.ld_gi = 64, 20
    if gemm == 1:
        d.X, d.ldx = ADDR, 20
    else:
        for name in ("rowPtr_fea", "columnIndex_fea", "values_fea", "rowPtr_xt", "columnIndex_xt", "values_xt"):
            setattr(d, name, ADDR)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _ws(L, d):
    return L.lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d))


def _status(L, d):
    """the status of the call itself, on a workspace of made-up address and ample size: the argument checks come first"""
    d.workspace, d.workspace_bytes = None, 0
    if L.lib.sgx_layer_backward_schedule(ctypes.byref(d)) >= 0:
        return L.lib.sgx_layer_backward(ctypes.byref(d), None)          # SGX_ERR_WORKSPACE: passed every argument check
    rc = L.lib.sgx_layer_backward(ctypes.byref(d), None)
    assert rc == L.lib.sgx_layer_backward_schedule(ctypes.byref(d)) and _ws(L, d) == 0
    return rc


def test_zeroed_new_fields_are_the_call_as_it_was(L):
    for gat in (0, 1):
        for gemm in (0, 1):
            base = _ws(L, _desc(L, gat, gemm))
            assert base > 0 and L.lib.sgx_layer_backward_schedule(ctypes.byref(_desc(L, gat, gemm))) == 0
            # capacities are read only under their flat schedule
            assert _ws(L, _desc(L, gat, gemm, nnz_fea=12345, nnz_xt=-7)) == base
    # the sizes of the layout before the fields existed (300 nodes, 2000 entries, M = 20, P = 64, fp32, E / S form)
    assert _ws(L, _desc(L, 0, 1)) == _expected_default(L, 0, 1) and _ws(L, _desc(L, 1, 0)) == _expected_default(L, 1, 0)


def _expected_default(L, gat, gemm):
    up = lambda b: -(-b // 256) * 256
    n, P, M, nnz = 300, 64, 20, 2000
    total = up(P * 4) + up(L.lib.sgx_col_sums_scratch_bytes(P)) + up(n * P * 4)
    if gat:
        if gemm == 1:
            total += up(P * M * 4)
        slices = min(max(-(-n // 64), 1), 1024)
        total += up(n * 64 * 4) + up((nnz + 1) * 4) + up(n * 4) + up(P * 4) + up(n * 16) + up(n * 4) + up(slices * 2 * P * 4)
    if gemm == 1:
        total += up(L.lib.sgx_xt_g_workspace_bytes(n, M, P))
    return total


def test_flat_workspace_is_the_default_plus_the_flat_scratches(L):
    spmm, ag = L.lib.sgx_spmm_flat_scratch_bytes, L.lib.sgx_gat_attention_grad_flat_workspace_bytes
    base = _ws(L, _desc(L))
    F = L.SGX_SCHEDULE_FLAT
    assert _ws(L, _desc(L, schedule_adj=F)) == base + spmm(2000, 64) + ag(2000, 300, 64)
    assert _ws(L, _desc(L, schedule_fea=F, nnz_fea=900)) == base + spmm(900, 64)
    assert _ws(L, _desc(L, schedule_xt=F, nnz_xt=901)) == base + spmm(901, 64)
    all3 = _ws(L, _desc(L, schedule_adj=F, schedule_fea=F, schedule_xt=F, nnz_fea=900, nnz_xt=901))
    assert all3 == base + spmm(2000, 64) + ag(2000, 300, 64) + spmm(900, 64) + spmm(901, 64)
    gcn = _ws(L, _desc(L, gat=0))
    assert _ws(L, _desc(L, gat=0, schedule_adj=F)) == gcn + spmm(2000, 64)              # no attention gradient
    last = 0
    for cap in (0, 1, 255, 256, 257, 2000, 70000, 1 << 24):                             # monotone in every capacity
        now = _ws(L, _desc(L, schedule_adj=F, schedule_fea=F, schedule_xt=F, nnz_adj=max(cap, 1), nnz_fea=cap, nnz_xt=cap))
        assert now >= last and now % 256 == 0
        last = now


def test_schedule_query_on_all_combinations(L):
    F = L.SGX_SCHEDULE_FLAT
    for bits in range(8):
        kw = dict(schedule_adj=F * (bits & 1), schedule_fea=F * (bits >> 1 & 1), schedule_xt=F * (bits >> 2 & 1), nnz_fea=50, nnz_xt=60)
        assert L.lib.sgx_layer_backward_schedule(ctypes.byref(_desc(L, 1, 0, **kw))) == bits
        assert L.lib.sgx_layer_backward_schedule(ctypes.byref(_desc(L, 0, 0, **kw))) == bits & 5       # GCN forms no Wh
        assert L.lib.sgx_layer_backward_schedule(ctypes.byref(_desc(L, 1, 1, **kw))) == bits & 1       # dense X: neither is read
    assert L.lib.sgx_layer_backward_schedule(None) == L.SGX_ERR_NULL


def test_layer_backward_refusals(L):
    F, U, S = L.SGX_SCHEDULE_FLAT, L.SGX_ERR_UNSUPPORTED, L.SGX_ERR_SHAPE
    assert _status(L, _desc(L)) == L.SGX_ERR_WORKSPACE
    assert _status(L, _desc(L, schedule_adj=F, schedule_fea=F, schedule_xt=F)) == L.SGX_ERR_WORKSPACE
    # a flat schedule together with the plan of the same matrix
    assert _status(L, _desc(L, schedule_adj=F, plan_adj=ADDR)) == U
    assert _status(L, _desc(L, schedule_fea=F, plan_fea=ADDR)) == U
    assert _status(L, _desc(L, schedule_xt=F, plan_xt=ADDR)) == U
    # neither enumerator
    for name in ("schedule_adj", "schedule_fea", "schedule_xt"):
        assert _status(L, _desc(L, **{name: 2})) == U and _status(L, _desc(L, **{name: -1})) == U
    # capacities
    assert _status(L, _desc(L, schedule_adj=F, nnz_adj=-1)) == S and _status(L, _desc(L, schedule_adj=F, nnz_adj=INT32_MAX + 1)) == S
    assert _status(L, _desc(L, schedule_adj=F, nnz_adj=INT32_MAX)) == L.SGX_ERR_WORKSPACE       # inside the range, as the stage calls have it
    assert _status(L, _desc(L, nnz_adj=INT32_MAX)) == U                                        # the default schedule, as before
    for name, cap in (("schedule_fea", "nnz_fea"), ("schedule_xt", "nnz_xt")):
        assert _status(L, _desc(L, **{name: F, cap: -1})) == S and _status(L, _desc(L, **{name: F, cap: INT32_MAX + 1})) == S
        assert _status(L, _desc(L, **{name: F, cap: 0})) == L.SGX_ERR_WORKSPACE
    # gemm_mode 1 reads neither schedule_fea nor schedule_xt, nor their capacities or plans
    d = _desc(L, 1, 1, schedule_fea=7, schedule_xt=-3, nnz_fea=-1, nnz_xt=-1)
    assert _status(L, d) == L.SGX_ERR_WORKSPACE
    d = _desc(L, 0, 0, schedule_fea=7)                                                  # GCN reads no feature CSR
    assert _status(L, d) == L.SGX_ERR_WORKSPACE
    # a workspace that is present but short, or off its boundary
    d = _desc(L, schedule_adj=F)
    need = _ws(L, d)
    d.workspace, d.workspace_bytes = ADDR, need - 1
    assert L.lib.sgx_layer_backward(ctypes.byref(d), None) == L.SGX_ERR_WORKSPACE
    d.workspace, d.workspace_bytes = ADDR + 64, need
    assert L.lib.sgx_layer_backward(ctypes.byref(d), None) == L.SGX_ERR_ALIGN


# ---- the rule in numpy -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [256, 128])
@pytest.mark.parametrize("F", [3, 64, 100])
def test_emulation_inside_the_bound_and_free_of_the_capacity(T, F):
    for name, deg in R.degree_cases(T).items():
        rp, ci, sg, g1 = R.build(deg, max(len(deg), 50), seed=len(name))
        Wh = (np.random.default_rng(F).random((max(len(deg), 50), F)) * 2 - 1).astype(np.float32)
        got = R.emulate(rp, ci, sg, g1, Wh, T)
        want, mag = R.exact(rp, ci, sg, g1, Wh)
        assert (np.abs(got - want) <= R.bound(rp, T, F, mag)).all(), name
        if int(rp[-1]) == 0:
            assert not got[F:].any() and not np.signbit(got[F:]).any()              # exactly +0
        # entries behind the end: NaN weights and columns out of range, at two capacities
        for extra in (1, 3 * T):
            ci2 = np.concatenate([ci, np.full(extra, 1 << 30, np.int32)])
            sg2 = np.concatenate([sg, np.full(extra, np.nan, np.float32)])
            assert np.array_equal(R.emulate(rp, ci2, sg2, g1, Wh, T).view(np.int32), got.view(np.int32)), (name, extra)
