"""The layers on the entry-split schedule, without a GPU: the new symbol, constants and struct fields in the derived
binding; sgx_layer_schedule on made-up addresses (it reads no device memory); every refused combination of
SGX_SCHEDULE_FLAT returned before memory is touched (the addresses are made up: touching them would fault); the workspace
size; the ValueErrors of ops.layer_forward(schedule=) and pyg_lite.NeighborLoader(schedule=)."""
import ctypes
import subprocess
import types

import pytest
import torch

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
F16, F32 = 0, 1


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _desc(L, **kw):
    """a dense-feature fp16 layer of 50 x 100 x 32 -> 64 on made-up addresses, under the flat schedule at 1000 entries"""
    d = L.LayerDesc(gemm_mode=1, N_adj=50, M_adj=100, M_fea=32, P_w=64, dtype=F16, B=0x10000, D=0x20000, values_fea=0x30000,
                    rowPtr_adj=0x40000, columnIndex_adj=0x50000, values_adj=0x60000, alpha=0.2,
                    schedule_adj=L.SGX_SCHEDULE_FLAT, nnz_adj=1000)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_binding(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    assert "sgx_layer_schedule" in L.SYMBOLS and " T sgx_layer_schedule\n" in out
    fn = L.lib.sgx_layer_schedule
    assert (fn.restype, list(fn.argtypes)) == (ctypes.c_int, [ctypes.POINTER(L.LayerDesc)])
    assert (L.SGX_SCHEDULE_DEFAULT, L.SGX_SCHEDULE_FLAT) == (0, 1)
    fields = dict(L.LayerDesc._fields_)
    assert fields["schedule_adj"] is ctypes.c_int32 and fields["nnz_adj"] is ctypes.c_int64
    names = [n for n, _ in L.LayerDesc._fields_]
    assert names[-3:] == ["order", "schedule_adj", "nnz_adj"]          # appended: every earlier offset is what it was
    zero = L.LayerDesc()
    assert zero.schedule_adj == 0 and zero.nnz_adj == 0                 # a zeroed descriptor is the layer as it was


def test_schedule_query(L):
    q = lambda d: L.lib.sgx_layer_schedule(ctypes.byref(d))
    for gat in (0, 1):
        kw = dict(gat_mode=gat, attention=0x70000 if gat else None)
        assert q(_desc(L, **kw)) == 2
        assert q(_desc(L, schedule_adj=0, **kw)) == 0
        assert q(_desc(L, schedule_adj=0, plan_adj=0x80000, **kw)) == 1
    assert q(_desc(L, gemm_mode=0, rowPtr_fea=0x90000, columnIndex_fea=0xA0000)) == 2
    assert q(_desc(L, gemm_mode=0, rowPtr_fea=0x90000, columnIndex_fea=0xA0000, plan_fea=0x80000)) == 2      # the X.W stage's plan stays
    assert q(_desc(L, dtype=F32)) == 2 and q(_desc(L, nnz_adj=0)) == 2 and q(_desc(L, nnz_adj=(1 << 31) - 1)) == 2
    assert q(_desc(L, M_fea=64)) == 2                                   # the square fp16 shape: staged under the flat schedule
    assert L.lib.sgx_layer_schedule(None) == NULL
    assert q(_desc(L, dtype=2)) == UNSUPPORTED and q(_desc(L, P_w=0)) == SHAPE       # the errors the call had before


def _refused(L):
    quant = L.Quant(qbits=8, internal_bits=8)
    return [
        ("plan_adj", dict(plan_adj=0x80000), UNSUPPORTED),
        ("quant", dict(dtype=F32, quant=ctypes.pointer(quant)), UNSUPPORTED),
        ("acc_mode", dict(acc_mode=L.SGX_ACC_REF_HALF), UNSUPPORTED),
        ("gat_heads", dict(gat_mode=1, attention=0x70000, gat_heads=2), UNSUPPORTED),
        ("E", dict(gat_mode=1, attention=0x70000, E=0xB0000), UNSUPPORTED),
        ("S", dict(gat_mode=1, attention=0x70000, S=0xC0000), UNSUPPORTED),
        ("E and S", dict(gat_mode=1, attention=0x70000, E=0xB0000, S=0xC0000), UNSUPPORTED),
        ("aggregate_first", dict(order=L.SGX_ORDER_AGGREGATE_FIRST), UNSUPPORTED),
        ("schedule_adj = 2", dict(schedule_adj=2), UNSUPPORTED),
        ("nnz_adj < 0", dict(nnz_adj=-1), SHAPE),
        ("nnz_adj > INT32_MAX", dict(nnz_adj=1 << 31), SHAPE),
    ]


def test_refused_combinations_touch_no_memory(L):
    """every pointer is made up and the workspace is large enough: a call that got past its checks would launch on them"""
    stats = L.GatStats(score_row=0x100000, score_col=0x101000, row_max=0x102000, row_sum=0x103000)
    for what, kw, status in _refused(L):
        d = _desc(L, workspace=0x1000000, workspace_bytes=1 << 30, **kw)
        assert L.lib.sgx_layer_schedule(ctypes.byref(d)) == status, what
        assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == status, what
        assert L.lib.sgx_layer_workspace_bytes(ctypes.byref(d)) == 0, what
        if d.gat_mode:
            assert L.lib.sgx_layer_forward_stats(ctypes.byref(d), ctypes.byref(stats), None) == status, what
    # each of them is accepted under the default schedule (nnz_adj is not read there)
    for what, kw, _ in _refused(L):
        if what.startswith("schedule_adj"):
            continue
        assert L.lib.sgx_layer_schedule(ctypes.byref(_desc(L, **{"schedule_adj": 0, **kw}))) in (0, 1), what


def test_workspace_accounts_for_the_flat_scratch(L):
    size = lambda d: L.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
    T = L.lib.sgx_spmm_flat_chunk()
    for dtype in (F16, F32):
        for P in (3, 64, 100):
            for M_fea in (32, 64):
                for gemm in (0, 1):
                    fea = dict(gemm_mode=gemm, rowPtr_fea=0x90000 if gemm == 0 else None, columnIndex_fea=0xA0000 if gemm == 0 else None)
                    last = 0
                    for nnz in (0, 1, T, T + 1, 3 * T, 1 << 20):
                        kw = dict(dtype=dtype, P_w=P, M_fea=M_fea, nnz_adj=nnz, **fea)
                        # the default size is the staged layer's: the fused square fp16 form, which needs none, is not the
                        # flat schedule's (SGX_LAYER_NO_FUSED_DENSE gives the same staged size under the default schedule)
                        staged = size(_desc(L, schedule_adj=0, **{**kw, "M_fea": 32 if (M_fea, P, dtype, gemm) == (64, 64, F16, 1) else M_fea}))
                        flat = L.lib.sgx_spmm_flat_scratch_bytes(nnz, P)
                        assert flat > 0 and size(_desc(L, **kw)) >= staged + flat >= last, (dtype, P, M_fea, gemm, nnz)
                        last = size(_desc(L, **kw))
                        for fill in (0, 1):
                            g = dict(gat_mode=1, attention=0x70000, gat_fill_dead_rows=fill, **kw)
                            gflat = L.lib.sgx_gat_flat_scratch_bytes(nnz, 50, 100, P, fill)
                            assert gflat > 0 and size(_desc(L, **g)) >= size(_desc(L, schedule_adj=0, **g)) + gflat, (g, nnz)


def _fact_csr(ops, flat=False, nnz=10):
    A = ops.Csr.__new__(ops.Csr)                                         # the facts alone: no device tensors here
    A._plan, A._max_row, A._flat, A._nnz = None, None, flat, nnz
    return A


def test_layer_forward_value_errors(L):
    from sgracex1_amd import ops
    A, X, Wt = _fact_csr(ops), torch.zeros(4, 8), torch.zeros(8, 8)
    with pytest.raises(ValueError, match="schedule must be None or 'flat'"):
        ops.layer_forward(A, X, Wt, schedule="rows")
    for kw, named in ((dict(quant=object()), "quant"), (dict(gat_heads=2, gat_attention=torch.zeros(16)), "gat_heads > 1"),
                      (dict(acc_mode=L.SGX_ACC_REF_HALF), "SGX_ACC_REF_HALF"),
                      (dict(want_edge_outputs=True, gat_attention=torch.zeros(16)), "want_edge_outputs"),
                      (dict(order="aggregate_first"), "aggregate_first")):
        with pytest.raises(ValueError, match=f"entry-split schedule does not go with .*{named}"):
            ops.layer_forward(A, X, Wt, schedule="flat", **kw)
        with pytest.raises(ValueError, match="entry-split schedule"):
            ops.layer_schedule(A, X, Wt, schedule="flat", **kw)
    # the fact is carried by the copies a layer makes of a matrix
    assert ops.Csr.with_facts(_fact_csr(ops), flat=True)._flat and not _fact_csr(ops)._flat


def test_neighbor_loader_value_errors(L):
    from sgracex1_amd import pyg_lite
    data = types.SimpleNamespace(x=None, edge_index=None)                # never looked at: the checks come first
    with pytest.raises(ValueError, match="schedule must be None or 'flat'"):
        pyg_lite.NeighborLoader(data, [3], schedule="rows", pad=True, prepare="sym_norm2")
    with pytest.raises(ValueError, match="schedule='flat' needs pad=True"):
        pyg_lite.NeighborLoader(data, [3], schedule="flat", prepare="sym_norm2")
    with pytest.raises(ValueError, match="quant=.*schedule='flat'"):
        pyg_lite.NeighborLoader(data, [3], schedule="flat", pad=True, prepare="sym_norm2", quant=object())
    with pytest.raises(ValueError, match="fan-outs >= 0"):
        pyg_lite.NeighborLoader(data, [100, -1], schedule="flat", pad=True, prepare="sym_norm2")
    with pytest.raises(ValueError, match=r"max\(num_neighbors\) \+ 1 <= 64"):           # without the keyword: as before
        pyg_lite.NeighborLoader(data, [100, 10], pad=True, prepare="sym_norm2")
