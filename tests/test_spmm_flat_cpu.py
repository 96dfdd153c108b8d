"""The entry-split aggregation without a GPU: the three symbols, every argument error of sgx_spmm_csr_flat on made-up
addresses (nothing is launched before the checks pass), the host checks of ops.spmm / Csr.with_facts(flat=True), and the
numpy restatement of the ownership rule (tests/_spmm_flat_ref.py) on the graphs of the GPU test: every row is stored by
exactly one (chunk, launch), every entry is read by exactly one chunk, the partial slots lie inside
sgx_spmm_flat_scratch_bytes, and the second launch adds exactly the slots the first one wrote for that row."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import _spmm_flat_ref as F

OK, NULL, SHAPE, UNSUPPORTED, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -7
F16, F32 = 0, 1


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_symbols(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    for name in ("sgx_spmm_flat_chunk", "sgx_spmm_flat_scratch_bytes", "sgx_spmm_csr_flat"):
        assert name in L.SYMBOLS and f" T {name}\n" in out
    assert (L.SGX_F16, L.SGX_F32) == (F16, F32)
    fn = L.lib.sgx_spmm_csr_flat
    assert (fn.restype, list(fn.argtypes)) == (i, [i, i, i, i, i, i64, vp, vp, vp, vp, i64, vp, i64, vp, ctypes.c_size_t, vp])
    assert (L.lib.sgx_spmm_flat_scratch_bytes.restype, list(L.lib.sgx_spmm_flat_scratch_bytes.argtypes)) == (ctypes.c_size_t, [i64, i])
    T = L.lib.sgx_spmm_flat_chunk()
    assert T >= 64 and T % 64 == 0                      # whole wavefront steps


def test_scratch_bytes(L):
    T, size = L.lib.sgx_spmm_flat_chunk(), L.lib.sgx_spmm_flat_scratch_bytes
    assert size(-1, 64) == 0 and size(10, 0) == 0 and size(1 << 31, 64) == 0
    for nnz, P in ((0, 1), (1, 3), (T, 64), (T + 1, 64), (10 * T + 5, 41), ((1 << 31) - 1, 520)):
        chunks = F.n_chunks(nnz, T)
        # two fp32 partial rows (pitch: P rounded up to 4) and two int32 per chunk, each region rounded up to 256 bytes
        want = -(-(chunks * 2 * (-(-P // 4) * 4) * 4) // 256) * 256 + -(-(chunks * 8) // 256) * 256
        assert size(nnz, P) == want, (nnz, P)


def _call(L, **kw):
    a = dict(dtype=F16, relu=0, n_rows=100, n_cols=50, n_feat=64, nnz=1000, rowPtr=0x10000, columnIndex=0x20000, values=0x30000,
             H=0x40000, ldh=64, D=0x50000, ldd=64, scratch=0x60000, scratch_bytes=None, stream=None)
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = L.lib.sgx_spmm_flat_scratch_bytes(max(a["nnz"], 0), max(a["n_feat"], 1))
    return L.lib.sgx_spmm_csr_flat(*a.values())


def test_argument_errors_need_no_gpu(L):
    for kw in (dict(n_rows=-1), dict(n_cols=-1), dict(n_feat=0), dict(ldh=63), dict(ldd=63), dict(nnz=-1), dict(nnz=1 << 31)):
        assert _call(L, **kw) == SHAPE, kw
    assert _call(L, dtype=2) == UNSUPPORTED
    assert _call(L, n_rows=0, rowPtr=None, D=None) == OK                 # nothing to store: nothing is looked at
    for kw in (dict(rowPtr=None), dict(D=None), dict(columnIndex=None), dict(values=None), dict(H=None)):
        assert _call(L, **kw) == NULL, kw
    # what nnz == 0 and n_cols == 0 excuse -- shown by the error behind them
    assert _call(L, nnz=0, columnIndex=None, values=None, H=None, scratch=None) == WORKSPACE
    assert _call(L, n_cols=0, H=None, scratch=None) == WORKSPACE
    # tables of 4 GiB and more, rows of 1 MiB and more
    assert _call(L, n_cols=1 << 25, ldh=64, H=0x40000) == UNSUPPORTED    # 2^25 x 64 x 2 bytes = 4 GiB
    assert _call(L, dtype=F32, n_cols=1 << 24, ldh=64) == UNSUPPORTED
    assert _call(L, n_feat=1 << 19, ldh=1 << 19, ldd=1 << 19, n_cols=2) == UNSUPPORTED
    assert _call(L, scratch=None) == WORKSPACE
    assert _call(L, scratch_bytes=L.lib.sgx_spmm_flat_scratch_bytes(1000, 64) - 1) == WORKSPACE
    assert _call(L, nnz=1025, scratch_bytes=L.lib.sgx_spmm_flat_scratch_bytes(1024, 64)) == WORKSPACE   # one chunk more
    for kw in (dict(scratch=0x60000 + 128), dict(rowPtr=0x10002), dict(columnIndex=0x20002), dict(values=0x30001), dict(H=0x40001),
               dict(D=0x50001), dict(dtype=F32, values=0x30002), dict(dtype=F32, H=0x40002), dict(dtype=F32, D=0x50002)):
        assert _call(L, **kw) == ALIGN, kw


def test_ops_host_checks(L):
    from sgracex1_amd import ops
    Csr = ops.Csr.__new__(ops.Csr)                                       # the facts alone: no device tensors here
    Csr._plan, Csr._max_row, Csr._flat, Csr._nnz = None, None, False, 1 << 21
    assert Csr.wants_plan
    assert Csr.with_facts(flat=True) is Csr and not Csr.wants_plan
    Csr._plan = object()
    assert Csr.wants_plan                                                # a plan that exists is still used where one is asked for
    Csr._plan = None
    assert Csr.with_facts(max_row=3)._flat and not Csr.with_facts(flat=False)._flat and Csr.wants_plan   # other facts leave it alone
    with pytest.raises(ValueError, match="schedule must be None or 'flat'"):
        ops.spmm(Csr, torch.zeros(4, 4), schedule="rows")
    with pytest.raises(ValueError, match="SGX_ACC_F32"):
        ops.spmm(Csr, torch.zeros(4, 4), schedule="flat", acc_mode=ops.SGX_ACC_REF_HALF)


@pytest.mark.parametrize("T", ["library", 128])
def test_ownership_rule(L, T):
    """The rule at the library's T and, to show it is the rule's and not the number's, at another (the graphs need T > 100)."""
    if T == "library":
        T = L.lib.sgx_spmm_flat_chunk()
    crossing_rows = 0
    for name, (deg, extra) in F.degree_cases(T).items():
        rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        n, end = len(deg), int(rp[-1])
        cap = end + extra
        s = F.schedule(rp, T, cap)
        assert s.n_chunks == F.n_chunks(cap, T), name
        # every row stored by exactly one (chunk, launch)
        assert sorted(r for r, _, _ in s.stores) == list(range(n)), name
        # every entry read by exactly one chunk, inside that chunk, as part of its own row
        seen = np.zeros(end, np.int64)
        for c, r, e0, e1 in s.reads:
            assert c * T <= e0 < e1 <= min((c + 1) * T, end) and rp[r] <= e0 and e1 <= rp[r + 1], (name, c, r)
            seen[e0:e1] += 1
        assert (seen == 1).all(), name
        # a row inside one chunk: launch 1, by the chunk that holds it (an empty row: its index, or the last live chunk)
        live_last = max(0, (end - 1) // T)
        for r, c, launch in s.stores:
            first, last = int(rp[r]), int(rp[r + 1]) - 1
            assert c == min(first // T, live_last), (name, r)
            assert launch == (2 if last >= first and last // T > c else 1), (name, r)
        # the partial slots: written once each, inside the scratch, and launch 2 adds exactly those of its row in chunk order
        slots = [slot for slot, _ in s.partials]
        assert len(slots) == len(set(slots)) and all(0 <= slot < 2 * s.n_chunks for slot in slots), name
        pitch = -(-64 // 4) * 4
        if T == L.lib.sgx_spmm_flat_chunk():                 # (the library sizes its scratch for its own T)
            assert (max(slots, default=-1) + 1) * pitch * 4 + s.n_chunks * 8 <= L.lib.sgx_spmm_flat_scratch_bytes(cap, 64), name
        by_row = {}
        for slot, r in s.partials:
            by_row.setdefault(r, []).append(slot)
        assert set(by_row) == set(s.sums) == {r for r, _, launch in s.stores if launch == 2}, name
        for r, added in s.sums.items():
            assert added == sorted(by_row[r], key=lambda slot: slot // 2) and [slot // 2 for slot in added] == list(
                range(int(rp[r]) // T, (int(rp[r + 1]) - 1) // T + 1)), (name, r)
            assert added[0] % 2 == 1 and all(slot % 2 == 0 for slot in added[1:]), (name, r)
        crossing_rows += len(s.sums)
        if name.startswith("long_"):
            assert max(len(v) for v in s.sums.values()) >= 6, name
    assert crossing_rows >= 8
