"""The quantised layers on the entry-split schedule, without a GPU: the two `_ep` declarations and SGX_QUANT_FLAT in the
header and the derived binding; sgx_layer_schedule and the workspace size of a flat descriptor with `quant` and the bit (made-up
addresses: neither reads device memory); the refusals that stay with the bit set, returned before memory is touched; the new
keywords of ops.layer_forward and NeighborLoader; the flat_quant fact on the copies a layer makes of a matrix."""
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3
F16, F32 = 0, 1
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgx.h")


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _quant(L, flat=True, **kw):
    q = L.Quant(qbits=8, scale_fea=4, internal_bits=16, flags=L.SGX_QUANT_FLAT if flat else 0, inv_scale_fea=255.0, inv_scale_w=127.0,
                inv_scale_adj=255.0, deq_factor=2.0, nnz_adj=1000, nnz_fea=700)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _desc(L, quant, **kw):
    """a dense-feature fp32 layer of 50 x 100 x 32 -> 64 on made-up addresses, under the flat schedule at 1000 entries"""
    d = L.LayerDesc(gemm_mode=1, N_adj=50, M_adj=100, M_fea=32, P_w=64, dtype=F32, B=0x10000, D=0x20000, values_fea=0x30000,
                    rowPtr_adj=0x40000, columnIndex_adj=0x50000, values_adj=0x60000, alpha=0.2,
                    schedule_adj=L.SGX_SCHEDULE_FLAT, nnz_adj=1000)
    d.quant = ctypes.pointer(quant) if quant is not None else None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_header_and_binding(L):
    text = open(HEADER).read()
    assert re.search(r"#define\s+SGX_QUANT_FLAT\s+8\b", text) and L.SGX_QUANT_FLAT == 8
    assert re.search(r"\bint\s+sgx_spmm_csr_flat_ep\(", text) and re.search(r"\bint\s+sgx_gat_aggregate_flat_ep\(", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_spmm_csr_flat_ep", "sgx_gat_aggregate_flat_ep"):
        assert name in L.SYMBOLS and f" T {name}\n" in out
    plain, ep = L.lib.sgx_spmm_csr_flat, L.lib.sgx_spmm_csr_flat_ep
    assert ep.restype is ctypes.c_int
    assert list(ep.argtypes) == list(plain.argtypes)[:-1] + [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    plain, ep = L.lib.sgx_gat_aggregate_flat, L.lib.sgx_gat_aggregate_flat_ep
    assert list(ep.argtypes) == list(plain.argtypes)[:-1] + [ctypes.c_float, ctypes.c_void_p]
    assert L.SGX_QUANT_FLAT & (L.SGX_QUANT_ADJ_DONE | L.SGX_QUANT_INT8 | L.SGX_QUANT_INT8_AUTO) == 0


def test_stage_calls_refuse_before_any_launch(L):
    """the requantising arguments are checked first: made-up addresses, a call past its checks would launch on them"""
    call = lambda dtype, s, sf, ib: L.lib.sgx_spmm_csr_flat_ep(dtype, 0, 5, 9, 4, 100, 0x1000, 0x2000, 0x3000, 0x4000, 4, 0x5000, 4,
                                                               0x10000, 1 << 20, s, sf, ib, None)
    assert call(F16, 0.0, 4, 16) == UNSUPPORTED                          # requantising is fp32-only
    assert call(F32, 2.0, -1, 16) == UNSUPPORTED and call(F32, 2.0, 31, 16) == UNSUPPORTED
    assert call(F32, 2.0, 4, -1) == UNSUPPORTED and call(F32, 2.0, 4, 31) == UNSUPPORTED
    assert call(2, 2.0, 0, 0) == UNSUPPORTED
    assert L.lib.sgx_spmm_csr_flat_ep(F32, 0, 0, 9, 4, 100, None, None, None, None, 4, None, 4, None, 0, 2.0, 4, 16, None) == OK    # no rows
    assert L.lib.sgx_gat_aggregate_flat_ep(F32, 0, 5, 9, 4, 2, 0.2, 100, 0x1000, 0x2000, 0x3000, 0x4000, 4, 0x6000, 0x5000, 4, None, 0,
                                           0x10000, 1 << 20, None, 2.0, None) == UNSUPPORTED                                       # two heads


def test_schedule_query(L):
    q = lambda d: L.lib.sgx_layer_schedule(ctypes.byref(d))
    on, off = _quant(L), _quant(L, flat=False)
    for gat in (0, 1):
        kw = dict(gat_mode=gat, attention=0x70000 if gat else None)
        assert q(_desc(L, on, **kw)) == 2
        assert q(_desc(L, off, **kw)) == UNSUPPORTED                     # without the bit: as before
        assert q(_desc(L, off, schedule_adj=0, **kw)) == 0 and q(_desc(L, on, schedule_adj=0, **kw)) == 0      # the bit is read nowhere else
        assert q(_desc(L, on, schedule_adj=0, plan_adj=0x80000, **kw)) == 1
    for flags in (L.SGX_QUANT_ADJ_DONE, L.SGX_QUANT_INT8, L.SGX_QUANT_INT8_AUTO):
        assert q(_desc(L, _quant(L, flags=L.SGX_QUANT_FLAT | flags))) == 2
        assert q(_desc(L, _quant(L, flags=flags))) == UNSUPPORTED
    assert q(_desc(L, on, gemm_mode=0, rowPtr_fea=0x90000, columnIndex_fea=0xA0000, plan_fea=0x80000)) == 2    # the X.W stage's plan stays


def test_workspace_is_the_default_layout_plus_the_flat_scratch(L):
    size = lambda d: L.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
    up = lambda x: (x + 255) // 256 * 256
    T = L.lib.sgx_spmm_flat_chunk()
    assert T == 256
    for P, M_fea, flags, gemm in ((3, 32, 0, 1), (64, 32, L.SGX_QUANT_ADJ_DONE, 1), (100, 144, L.SGX_QUANT_INT8_AUTO, 1), (64, 20, 0, 0)):
        fea = dict(gemm_mode=gemm, rowPtr_fea=0x90000 if gemm == 0 else None, columnIndex_fea=0xA0000 if gemm == 0 else None)
        for nnz in (0, 1, T, T + 1, 3 * T):
            on = _quant(L, flags=L.SGX_QUANT_FLAT | flags, nnz_adj=nnz)
            off = _quant(L, flags=flags, nnz_adj=nnz)
            kw = dict(P_w=P, M_fea=M_fea, nnz_adj=nnz, **fea)
            base = size(_desc(L, off, schedule_adj=0, **kw))
            assert base > 0 and size(_desc(L, off, **kw)) == 0
            assert size(_desc(L, on, **kw)) == up(base) + up(L.lib.sgx_spmm_flat_scratch_bytes(nnz, P)), (P, M_fea, flags, gemm, nnz)
            for fill in (0, 1):
                g = dict(gat_mode=1, attention=0x70000, gat_fill_dead_rows=fill, **kw)
                gbase = size(_desc(L, off, schedule_adj=0, **g))
                want = up(gbase) + up(L.lib.sgx_gat_flat_scratch_bytes(nnz, 50, 100, P, fill))
                assert gbase > 0 and size(_desc(L, on, **g)) == want, (P, M_fea, flags, gemm, nnz, fill)


def _refused(L):
    return [
        ("plan_adj", dict(plan_adj=0x80000)),
        ("gat_heads", dict(gat_mode=1, attention=0x70000, gat_heads=2)),
        ("E", dict(gat_mode=1, attention=0x70000, E=0xB0000)),
        ("S", dict(gat_mode=1, attention=0x70000, S=0xC0000)),
        ("aggregate_first", dict(order=L.SGX_ORDER_AGGREGATE_FIRST)),
        ("dtype F16", dict(dtype=F16)),
        ("acc_mode", dict(acc_mode=L.SGX_ACC_REF_HALF)),
    ]


def test_refusals_kept_with_the_bit_touch_no_memory(L):
    """every pointer is made up and the workspace is large enough: a call that got past its checks would launch on them"""
    stats = L.GatStats(score_row=0x100000, score_col=0x101000, row_max=0x102000, row_sum=0x103000)
    on = _quant(L)
    for what, kw in _refused(L) + [("no bit", dict())]:
        d = _desc(L, _quant(L, flat=False) if what == "no bit" else on, workspace=0x1000000, workspace_bytes=1 << 30, **kw)
        assert L.lib.sgx_layer_schedule(ctypes.byref(d)) == UNSUPPORTED, what
        assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == UNSUPPORTED, what
        assert L.lib.sgx_layer_workspace_bytes(ctypes.byref(d)) == 0, what
        if d.gat_mode:
            assert L.lib.sgx_layer_forward_stats(ctypes.byref(d), ctypes.byref(stats), None) == UNSUPPORTED, what
    # the quantiser's own range checks hold on this route too
    for kw in (dict(internal_bits=0), dict(scale_fea=31), dict(qbits=17), dict(zero_adj=1.0)):
        d = _desc(L, _quant(L, **kw), workspace=0x1000000, workspace_bytes=1 << 30)
        assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == UNSUPPORTED, kw


def _fact_csr(ops, flat=False, flat_quant=False, nnz=10):
    A = ops.Csr.__new__(ops.Csr)                                         # the facts alone: no device tensors here
    A._plan, A._max_row, A._flat, A._flat_quant, A._nnz = None, None, flat, flat_quant, nnz
    return A


def test_layer_forward_keyword(L):
    """quant_flat=True takes `quant` off the list of what the keyword refuses -- the call then gets as far as its operand
    checks (a float16 weight matrix: the quantised layer's own TypeError) -- and nothing else"""
    from sgracex1_amd import ops, quant
    qc = quant.constants(8)
    A, X, Wt = _fact_csr(ops), torch.zeros(4, 8), torch.zeros(8, 8)
    with pytest.raises(ValueError, match="entry-split schedule does not go with .*quant"):
        ops.layer_forward(A, X, Wt, schedule="flat", quant=qc)
    with pytest.raises(ValueError, match="entry-split schedule does not go with .*quant"):
        ops.layer_forward(_fact_csr(ops, True, True), X, Wt, schedule="flat", quant=qc)      # the keyword wants its own opt-in
    with pytest.raises(ValueError, match="Wt must be a tensor on the GPU"):
        ops.layer_forward(A, X, Wt, schedule="flat", quant=qc, quant_flat=True)
    with pytest.raises(ValueError, match="Wt must be a tensor on the GPU"):
        ops.layer_forward(_fact_csr(ops, True, True), X, Wt, quant=qc)                       # the pair of facts opts in too
    with pytest.raises(ValueError, match="Wt must be a tensor on the GPU"):
        ops.layer_schedule(A, X, Wt, schedule="flat", quant=qc, quant_flat=True)
    with pytest.raises(ValueError, match="entry-split schedule does not go with gat_heads > 1"):
        ops.layer_forward(A, X, Wt, schedule="flat", quant=qc, quant_flat=True, gat_heads=2, gat_attention=torch.zeros(16))
    with pytest.raises(ValueError, match="entry-split schedule does not go with want_edge_outputs"):
        ops.layer_schedule(A, X, Wt, schedule="flat", quant=qc, quant_flat=True, want_edge_outputs=True, gat_attention=torch.zeros(16))


def test_stage_keywords_need_the_flat_form(L):
    from sgracex1_amd import ops
    A, H = _fact_csr(ops), torch.zeros(4, 8)
    with pytest.raises(ValueError, match="out_scale / requant"):
        ops.spmm(A, H, out_scale=2.0)
    with pytest.raises(ValueError, match="out_scale / requant"):
        ops.spmm(A, H, requant=(4, 16))
    with pytest.raises(TypeError, match="requant works on float32"):
        ops.spmm(A, H.half(), schedule="flat", requant=(4, 16))
    with pytest.raises(ValueError, match="out_scale is the entry-split form's epilogue"):
        ops.gat_aggregate(A, H, torch.zeros(16), out_scale=2.0)


def test_fact_is_carried(L):
    from sgracex1_amd import ops, quant
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    mk = lambda: ops.Csr.__new__(ops.Csr)
    A = mk()
    A.rowptr, A.col, A.val, A.n_rows, A.n_cols, A._nnz = rp, torch.zeros(3, dtype=torch.int32), torch.ones(3), 2, 2, 3
    A._plan = A._max_row = A._dead_rows = A._dead_row_mask = A._dead_rows_version = A._dead_row_mask_version = None
    A._flat, A._flat_quant, A._quantized = False, False, {}
    assert A.with_facts(flat=True, flat_quant=True) is A and A._flat and A._flat_quant
    assert A.with_facts(max_row=3)._flat_quant                            # another fact leaves it alone
    assert A.to(torch.float32) is A
    # the copies a layer makes: Csr.to, Csr.quantized and ops.csr_transpose hand the pair of facts on (the constructors
    # they call want device tensors: their bodies are followed on stand-ins)
    made = []
    real = ops.Csr

    class Stub:
        def __init__(self, rowptr, col, val, n_cols, plan=None):         # (Csr's own signature: a call that drifts from it fails here)
            assert rowptr is A.rowptr and col is A.col and n_cols == A.n_cols and plan is None
            made.append(self)
            self._flat = self._flat_quant = False
            self._max_row = None

        with_facts = real.with_facts
    try:
        ops.Csr = Stub
        ops.fake_quantize, fq = (lambda *a, **k: None), ops.fake_quantize
        B = real.to(A, torch.float16)
        Qm = real.quantized(A, quant.constants(8))
    finally:
        ops.Csr, ops.fake_quantize = real, fq
    assert len(made) == 2 and B._flat and B._flat_quant and Qm._flat and Qm._flat_quant
    Tm = _fact_csr(ops)
    Tm.n_rows = 0
    assert ops._transposed(Tm, False, None, A._flat, A._flat_quant) is Tm and Tm._flat and Tm._flat_quant
    plain = _fact_csr(ops)
    plain.n_rows = 0
    assert not ops._transposed(plain, False, None, True)._flat_quant and plain._flat


def test_neighbor_loader_keyword(L):
    from sgracex1_amd import pyg_lite, quant
    data = types.SimpleNamespace(x=None, edge_index=None)                # never looked at: the checks come first
    qc = quant.constants(8)
    kw = dict(pad=True, prepare="sym_norm2", schedule="flat")
    with pytest.raises(ValueError, match="quant=.*schedule='flat'"):
        pyg_lite.NeighborLoader(data, [100, 10], quant=qc, **kw)
    with pytest.raises(ValueError, match="flat_quant=True needs schedule='flat' and quant="):
        pyg_lite.NeighborLoader(data, [100, 10], flat_quant=True, **kw)
    with pytest.raises(ValueError, match="flat_quant=True needs schedule='flat' and quant="):
        pyg_lite.NeighborLoader(data, [10], quant=qc, flat_quant=True, pad=True, prepare="sym_norm2")
    # the padded quantised loader's host checks: a filler row's diagonal 1 must stay positive, its spare 0 must stay 0
    import dataclasses
    dead = dataclasses.replace(qc, a_s=4.0)                              # fq(1) = round(0.25) / 128 = 0
    with pytest.raises(ValueError, match=r"pad=True with quant=: with quant's a_s .* a filler row's diagonal 1 rounds to 0"):
        pyg_lite.NeighborLoader(data, [100, 10], quant=dead, flat_quant=True, **kw)
    shifted = dataclasses.replace(qc, a_z=3)                             # fq(0) = 3 / 128
    with pytest.raises(ValueError, match=r"pad=True with quant=: with quant's a_s .* a filler row's spare 0 becomes .*carry weight"):
        pyg_lite.NeighborLoader(data, [100, 10], quant=shifted, flat_quant=True, **kw)
