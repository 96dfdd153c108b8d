"""The net under tests/test_gpu_xw_dense_arms.py, checked without a GPU (tests/_xw_dense_ref.py): sgx_xw_dense_form -- the
host query the launch's own functions answer -- names, for every case of the table, the arm the case is there for, and the
arms reached are exactly the list the table is built for, so a moved gate fails here before any GPU run; and the float64
reference with its bound has no slack where it matters: every mutation a dense-product kernel could suffer puts EVERY row
it touches outside 2 x bound in at least one column (a GPU result is within 1 x bound of float64, so such a mutation cannot
hide behind the kernel's own rounding)."""
import ctypes

import numpy as np
import pytest

import _spmm_acc_ref as R
import _xw_dense_ref as D

ES = {"f16": 2, "f32": 4}
BASE = 1 << 20                      # a stand-in address: only the alignment of a pointer is read


def _lib():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _form(L, case, n=None, **tune):
    from sgracex1_amd import ops
    import torch
    n = case.n if n is None else n
    ldx, xs, ldw, ws, ldh, hs = D.layout(case)
    es = ES[case.dt]
    ptr = lambda base, skip: ctypes.c_void_p(base + skip * es)
    with L.tuning(**{k: "1" for k in case.env}, **tune):
        word = L.lib.sgx_xw_dense_form(L.SGX_F16 if case.dt == "f16" else L.SGX_F32, L.SGX_ACC_F32, n, case.M, case.P,
                                       ptr(BASE, xs), ldx, ptr(2 * BASE, ws), ldw, ptr(3 * BASE, hs), ldh)
    return ops.unpack_xw_dense_form(word, torch.float16 if case.dt == "f16" else torch.float32, n)


def test_the_table_reaches_exactly_the_arms_it_is_built_for():
    L = _lib()
    seen = set()
    for c in D.CASES:
        f = _form(L, c)
        assert (f.kind, f.a, f.b) == c.arm and f.blocks == c.blocks, (c.name, f)
        assert f.max_trips >= c.trips and f.max_trips == D.max_trips(c, f.waves, f.blocks), (c.name, f)
        assert c.wgs is None or f.wgs_per_cu == c.wgs, (c.name, f)
        if c.trips == 1 and f.kind in ("stationary", "wlds"):
            assert f.max_trips <= 2, (c.name, f)                    # many trips only where they are the point
        seen.add((c.dt, f.kind, f.a, f.b))
        chunk = _form(L, c, n=min(c.n, D.CHUNK))
        assert chunk.kind == "tile" and chunk.max_trips == 1, (c.name, chunk)          # the bits' reference: under every gate
    assert seen == D.ARMS, (sorted(seen - D.ARMS), sorted(D.ARMS - seen))


def test_the_gates_sit_where_the_table_says():
    L = _lib()
    c = D.BY_NAME["h_st_2x8_gate"]
    assert c.n == 8192 and _form(L, c, n=8191).kind == "tile" and _form(L, c).kind == "stationary"
    assert D.BY_NAME["h_tile_under_gate"].n == 8191
    c = D.BY_NAME["h_wlds_2"]
    assert c.n == 32768 and _form(L, c, n=32767)[:3] == ("tile", 2, 4) and _form(L, c).kind == "wlds"
    # the overrides lead where the GPU test expects them to
    assert _form(L, D.BY_NAME["h_wlds_4"], SGX_XW_NO_WLDS="1").kind == "tile_lds"
    assert _form(L, D.BY_NAME["h_wlds_4"], SGX_XW_NO_LDS="1")[:3] == ("tile", 4, 4)
    assert _form(L, D.BY_NAME["h_tall_8x4"], SGX_XW_SHORT_TILES="1")[:3] == ("tile", 8, 2)
    assert _form(L, D.BY_NAME["f_wlds_8x16"], SGX_XW_NO_WLDS="1")[:3] == ("stationary", 8, 4)
    assert _form(L, D.BY_NAME["f_wlds_8x16"], SGX_XW_NO_WLDS="1", SGX_XW_NO_STATIONARY_F32="1")[:3] == ("tile", 16, 2)
    assert _form(L, D.BY_NAME["f_tall_16x2"], SGX_XW_SHORT_TILES="1")[:3] == ("tile", 16, 1)
    # the idle wavefront of the five-group case: the grid's whole workgroups hold one wavefront more than the groups use
    f = _form(L, D.BY_NAME["h_st_trips"])
    assert f.waves == 8196 and f.blocks == 5 and f.waves % f.blocks == 1 and f.max_trips == 3
    assert (D.BY_NAME["h_st_trips"].n + 31) // 32 % (f.waves // 5) != 0                # a ragged last trip
    # three column groups (K in 65..128, P = 192) on a saturated grid: 8193 wavefronts wanted, 2049 workgroups hold 8196, and
    # the kernel makes 8196 / 3 = 2732 streams of them, not 2731 -- the form counts as the kernel does
    c = D.BY_NAME["h_st_4x4"]._replace(n=262144 + 37, P=192)
    f = _form(L, c)
    assert f[:3] == ("stationary", 4, 4) and f.blocks == 3 and f.waves == 8196 and f.waves % 4 == 0
    assert f.max_trips == -(-((c.n + 31) // 32) // 2732) == D.max_trips(c, f.waves, f.blocks) == 3
    # vector stores: every case of the table but the guard's variants (test_gpu_xw_dense_arms.py) stores by vectors
    assert all(_form(L, c).vec for c in D.CASES)


def test_query_answers_what_the_call_would_refuse():
    L = _lib()
    q = L.lib.sgx_xw_dense_form
    p = ctypes.c_void_p(BASE)
    assert q(L.SGX_F16, L.SGX_ACC_F32, 4, 0, 8, p, 8, p, 8, p, 8) == L.SGX_ERR_SHAPE
    assert q(L.SGX_F16, L.SGX_ACC_F32, 4, 8, 8, p, 8, p, 8, p, 7) == L.SGX_ERR_SHAPE
    assert q(L.SGX_F16, L.SGX_ACC_F32, 4, 8, 8, None, 8, p, 8, p, 8) == L.SGX_ERR_NULL
    assert q(7, L.SGX_ACC_F32, 4, 8, 8, p, 8, p, 8, p, 8) == L.SGX_ERR_UNSUPPORTED
    assert q(L.SGX_F32, L.SGX_ACC_REF_HALF, 4, 8, 8, p, 8, p, 8, p, 8) == L.SGX_ERR_UNSUPPORTED
    assert q(L.SGX_F16, L.SGX_ACC_REF_HALF, 4, 8, 8, p, 8, p, 8, p, 8) == L.SGX_XW_FORM_REF_HALF
    assert q(L.SGX_F16, L.SGX_ACC_F32, 0, 8, 8, None, 8, None, 8, None, 8) == L.SGX_XW_FORM_NONE


def test_pitch_restated():
    from sgracex1_amd import ops
    for c in D.CASES:
        assert D.pitch(c.P, c.dt) == ops.table_pitch(c.P, ES[c.dt])


M_SMALL, M_LARGE = min(c.M for c in D.CASES), max(c.M for c in D.CASES)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("M", [M_SMALL, M_LARGE])
def test_mutations_land_outside_the_bound(M, dt):
    assert M_SMALL == 7 and M_LARGE >= 602
    n, P = 80, 64
    X, Wt = D.operands(n, M, P, dt)
    X64, W64 = X.astype(np.float64), Wt.astype(np.float64)
    assert np.abs(X64).min() >= 0.25 and np.abs(W64).min() >= 0.25 and np.abs(X64).max() <= 1 and np.abs(W64).max() <= 1
    want, bound = D.reference(X, Wt, dt)
    assert np.array_equal(bound, D.bound(M, np.abs(X64) @ np.abs(W64).T, want, dt)) and np.array_equal(
        D.bound(M, 0.0 * want, want, dt), R.store_bound(want, dt))         # (the house store term of _spmm_acc_ref)

    def caught(what, rows, mutated):
        out = (np.abs(mutated - want[rows]) > 2.0 * bound[rows]).any(1)
        assert len(out) > 0 and out.all(), f"M = {M} {dt}: {what}: {int((~out).sum())} of {len(out)} mutated rows stay inside the bound"

    every = np.arange(n)
    caught("a row's last k dropped", every, want - X64[:, -1:] * W64[None, :, -1])
    # the ring's hazard: the lanes of a row's last k-step past M hold the next row's first elements (of X and, in the copy
    # of W^T, of the next column's row)
    rows = every[:-1]
    caught("the next row's first element added at k = M", rows, want[rows] + X64[rows + 1, :1] * np.roll(W64[:, 0], -1)[None, :])
    step = D.k_step(dt)
    ks = slice(step, 2 * step) if M > step else slice(0, M)
    caught(f"one k-step of {step} skipped", every, want - X64[:, ks] @ W64[:, ks].T)
    swapped = want.reshape(n, P // 2, 2)[:, :, ::-1].reshape(n, P)
    caught("the two columns of a pair swapped", every, swapped)
    swapped = want.reshape(n, P // 8, 2, 4)[:, :, ::-1].reshape(n, P)
    caught("the two tiles of a pair swapped (4 + 4 columns)", every, swapped)
    caught("row m stored at m + 16", every[16:], want[:-16])
