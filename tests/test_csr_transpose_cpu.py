"""sgx_csr_transpose without a GPU: the two symbols, the header's declarations against the binding, every argument error --
all of which come back before anything reaches a device --, the workspace size, and the numpy restatement of the rule
(tests/_transpose_ref.py) against a dense transpose."""
import os
import re
import subprocess

import numpy as np
import pytest

import _transpose_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgx.h")
NULL, SHAPE, UNSUPPORTED, WORKSPACE, ALIGN = -1, -2, -3, -4, -7
PTR = 4096            # a non-NULL, aligned stand-in: no call below gets as far as reading through a pointer
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_new_symbols_exist(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_csr_transpose_workspace_bytes", "sgx_csr_transpose"):
        assert name in L.SYMBOLS and f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^(\w[\w \*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text, flags=re.M)
    assert m, f"{name} is not declared in include/sgx.h"
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def test_header_declares_them_and_the_binding_matches(L):
    ret, args = _declaration("sgx_csr_transpose_workspace_bytes")
    assert ret == "size_t" and len(args) == 3 == len(L.lib.sgx_csr_transpose_workspace_bytes.argtypes)
    ret, args = _declaration("sgx_csr_transpose")
    assert ret == "int" and len(args) == 14 == len(L.lib.sgx_csr_transpose.argtypes)
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "dtype_values", "n_rows", "n_cols", "nnz", "rowPtr", "columnIndex", "values", "rowPtr_t", "columnIndex_t", "values_t",
        "order", "workspace", "workspace_bytes", "stream"]
    tile = int(re.search(r"#define\s+SGX_CSR_TRANSPOSE_TILE\s+(\d+)", open(HEADER).read()).group(1))
    assert tile == L.SGX_CSR_TRANSPOSE_TILE and tile % 256 == 0
    # the additions stand behind everything the header held before: nothing above them changed place
    text = open(HEADER).read()
    assert text.index("sgx_csr_transpose") > text.index("int    sgx_layer_backward(")


NAMES = ("dtype", "n_rows", "n_cols", "nnz", "rowPtr", "columnIndex", "values", "rowPtr_t", "columnIndex_t", "values_t", "order",
         "ws", "ws_bytes", "stream")


def _call(L, **kw):
    n_rows, n_cols, nnz = kw.get("n_rows", 100), kw.get("n_cols", 300), kw.get("nnz", 5000)
    need = L.lib.sgx_csr_transpose_workspace_bytes(max(n_rows, 0), max(n_cols, 0), min(max(nnz, 0), INT32_MAX))
    ok = dict(dtype=L.SGX_F32, n_rows=100, n_cols=300, nnz=5000, rowPtr=PTR, columnIndex=PTR, values=PTR, rowPtr_t=PTR,
              columnIndex_t=PTR, values_t=PTR, order=PTR, ws=PTR, ws_bytes=need, stream=None)
    ok.update(kw)
    return L.lib.sgx_csr_transpose(*[ok[n] for n in NAMES])


def test_argument_errors_come_back_before_a_device_call(L):
    # (an accepted call would launch: every call below is refused, the last checks being the workspace's)
    for name in ("rowPtr", "columnIndex", "rowPtr_t", "columnIndex_t"):
        assert _call(L, **{name: None}) == NULL, name
    assert _call(L, values=None) == NULL and _call(L, values_t=None) == NULL          # exactly one of the pair
    assert _call(L, n_rows=-1) == SHAPE and _call(L, n_cols=-1) == SHAPE and _call(L, nnz=-1) == SHAPE
    assert _call(L, nnz=INT32_MAX + 1) == UNSUPPORTED
    assert _call(L, dtype=5) == UNSUPPORTED and _call(L, dtype=-1) == UNSUPPORTED
    need = L.lib.sgx_csr_transpose_workspace_bytes(100, 300, 5000)
    assert _call(L, ws=None) == WORKSPACE and _call(L, ws_bytes=need - 1) == WORKSPACE and _call(L, ws_bytes=0) == WORKSPACE
    assert _call(L, ws=PTR + 16) == ALIGN
    # with both value arrays NULL the dtype is not looked at, and order is optional: such a call gets as far as its workspace
    assert _call(L, values=None, values_t=None, dtype=5, ws=None) == WORKSPACE
    assert _call(L, values=None, values_t=None, dtype=5, ws=PTR + 16) == ALIGN
    assert _call(L, order=None, ws=PTR + 16) == ALIGN
    # fp16 values are accepted
    assert _call(L, dtype=L.SGX_F16, ws=PTR + 16) == ALIGN
    # the empty shapes are valid calls: they too get as far as the workspace
    assert _call(L, n_rows=0, nnz=0, ws=None) == WORKSPACE and _call(L, nnz=0, n_cols=5, ws=PTR + 16) == ALIGN
    # the largest entry count is accepted up to its workspace
    assert _call(L, nnz=INT32_MAX, ws_bytes=1024) == WORKSPACE


def test_workspace_bytes(L):
    f = L.lib.sgx_csr_transpose_workspace_bytes
    assert f(-1, 5, 10) == 0 and f(5, -1, 10) == 0 and f(5, 5, -1) == 0 and f(5, 5, INT32_MAX + 1) == 0
    tile = L.SGX_CSR_TRANSPOSE_TILE
    last = 0
    for nnz in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 10 * tile, 10 ** 6, 10 ** 8, INT32_MAX):
        need = f(1000, 1000, nnz)
        assert need > 0 and need % 256 == 0 and need >= last, nnz
        assert need >= 2 * 4 * nnz                      # at least the sort's two position buffers
        last = need
    assert f(0, 0, 0) > 0 and f(0, 5, 0) % 256 == 0


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 12), (40, 3, 60), (3, 40, 60), (64, 64, 700), (17, 300, 900)])
def test_restatement_is_the_dense_transpose(shape):
    n_rows, n_cols, nnz = shape
    rng = np.random.default_rng(n_rows * 1000 + n_cols)
    rowptr, col, val = TR.random_csr(rng, n_rows, n_cols, nnz, unique=True)
    dense = np.zeros((n_rows, n_cols), np.float32)
    row = np.repeat(np.arange(n_rows), np.diff(rowptr))
    dense[row, col] = val
    rp_t, col_t, val_t, order = TR.transpose(rowptr, col, val, n_cols)
    # the CSR of dense.T, rows by rows, ascending columns
    want_r, want_c = np.nonzero(dense.T)
    assert np.array_equal(np.repeat(np.arange(n_cols), np.diff(rp_t)), want_r) and np.array_equal(col_t, want_c)
    assert np.array_equal(val_t, dense.T[want_r, want_c]) and np.array_equal(val[order], val_t)
    assert rp_t[0] == 0 and rp_t[-1] == len(col) and len(rp_t) == n_cols + 1
    # twice is the identity on such a matrix
    rp2, col2, val2, _ = TR.transpose(rp_t, col_t, val_t, n_rows)
    assert np.array_equal(rp2, rowptr) and np.array_equal(col2, col) and np.array_equal(val2, val)


def test_restatement_is_stable_on_repeated_pairs():
    rowptr = np.array([0, 3, 3, 6], np.int32)
    col = np.array([2, 0, 2, 2, 2, 0], np.int32)         # row 0: (2, 0, 2), row 2: (2, 2, 0); column 1 empty
    val = np.arange(6, dtype=np.float32)
    rp_t, col_t, val_t, order = TR.transpose(rowptr, col, val, 4)
    assert rp_t.tolist() == [0, 2, 2, 6, 6] and order.tolist() == [1, 5, 0, 2, 3, 4]
    assert col_t.tolist() == [0, 2, 0, 0, 2, 2] and val_t.tolist() == [1, 5, 0, 2, 3, 4]
