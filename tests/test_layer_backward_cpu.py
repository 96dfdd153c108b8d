"""The one-call layer backward without a GPU: the new symbols, the layout of sgx_layer_grad_desc against its ctypes mirror,
every argument error of sgx_layer_backward and sgx_gat_attention_grad -- all of which come back before anything reaches a
device -- and a workspace size of 0 for a descriptor the call refuses."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, UNSUPPORTED, WORKSPACE, ALIGN = -1, -2, -3, -4, -7
PTR = 4096            # a non-NULL, aligned stand-in: no call below gets as far as reading through a pointer


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _desc(L, gat=1, gemm=1, form="es"):
    """A descriptor the call accepts up to its workspace."""
    d = L.LayerGradDesc()
    d.gat_mode, d.gemm_mode, d.N_adj, d.M_adj, d.M_fea, d.P_w = gat, gemm, 100, 100, 7, 16
    d.dtype_adj, d.dtype_x, d.gat_heads, d.alpha, d.nnz_adj = L.SGX_F32, L.SGX_F32, 1, 0.2, 1000
    d.rowPtr_adj = d.columnIndex_adj = d.values_adj = PTR
    d.W = d.G = d.grad_weights = d.grad_input = PTR
    d.ldg, d.ld_gi = 16, 8
    if gemm == 1:
        d.X, d.ldx = PTR, 7
    else:
        d.rowPtr_xt = d.columnIndex_xt = d.values_xt = PTR
        d.rowPtr_fea = d.columnIndex_fea = d.values_fea = PTR
    if gat:
        d.grad_attention = PTR
        if form == "es":
            d.E = d.S = PTR
    return d


def test_new_symbols_exist(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_layer_backward_workspace_bytes", "sgx_layer_backward", "sgx_gat_attention_grad",
                 "sgx_gat_attention_grad_workspace_bytes"):
        assert name in L.SYMBOLS and f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110


def test_struct_layout_matches_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
                   ' printf("sizeof %zu\\n", sizeof(sgx_layer_grad_desc));\n'
                   + "".join(f' printf("{n} %zu\\n", offsetof(sgx_layer_grad_desc, {n}));\n' for n, _ in L.LayerGradDesc._fields_)
                   + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            name, v = ln.split()
            seen += 1
            if name == "sizeof":
                assert ctypes.sizeof(L.LayerGradDesc) == int(v)
            else:
                assert getattr(L.LayerGradDesc, name).offset == int(v), name
    assert seen == 1 + len(L.LayerGradDesc._fields_)


def _refused(L, d, status):
    assert L.lib.sgx_layer_backward(ctypes.byref(d), None) == status
    assert L.lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d)) == 0


def test_argument_errors_come_back_before_a_device_call(L):
    lib = L.lib
    assert lib.sgx_layer_backward(None, None) == NULL and lib.sgx_layer_backward_workspace_bytes(None) == 0
    # an accepted descriptor: a positive size, a multiple of 256; then the workspace errors
    for gat, gemm, form in ((1, 1, "es"), (1, 0, "es"), (0, 1, None), (0, 0, None)):
        d = _desc(L, gat, gemm, form)
        need = lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d))
        assert need > 0 and need % 256 == 0
        assert lib.sgx_layer_backward(ctypes.byref(d), None) == WORKSPACE               # none given
        d.workspace, d.workspace_bytes = PTR, need - 1
        assert lib.sgx_layer_backward(ctypes.byref(d), None) == WORKSPACE               # too small
        d.workspace, d.workspace_bytes = PTR + 128, need
        assert lib.sgx_layer_backward(ctypes.byref(d), None) == ALIGN
    # grad_input is optional; without it the size does not grow
    d = _desc(L)
    with_gi = lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d))
    d.grad_input = None
    assert 0 < lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d)) <= with_gi
    # shape
    for field, value in (("N_adj", 0), ("M_fea", 0), ("P_w", 0), ("nnz_adj", -1), ("M_adj", 99), ("ldg", 15), ("ldx", 6),
                         ("ld_gi", 6)):
        d = _desc(L)
        setattr(d, field, value)
        _refused(L, d, SHAPE)
    # unsupported: heads, modes, element types
    for field, value in (("gat_heads", 2), ("gat_mode", 2), ("gemm_mode", 2), ("dtype_adj", 5), ("dtype_x", 5)):
        d = _desc(L)
        setattr(d, field, value)
        _refused(L, d, UNSUPPORTED)
    # required pointers, per mode
    for field in ("rowPtr_adj", "columnIndex_adj", "values_adj", "W", "G", "grad_weights", "X", "grad_attention", "E", "S"):
        d = _desc(L)
        setattr(d, field, None)
        _refused(L, d, NULL)
    for field in ("rowPtr_xt", "columnIndex_xt", "values_xt", "rowPtr_fea", "columnIndex_fea", "values_fea"):
        d = _desc(L, 1, 0)
        setattr(d, field, None)
        _refused(L, d, NULL)
    d = _desc(L, 0, 0)                                   # GCN reads no CSR of X, only of X^T
    d.rowPtr_fea = d.columnIndex_fea = d.values_fea = None
    assert lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d)) > 0
    # the forward's state: one form
    d = _desc(L, form=None)
    _refused(L, d, NULL)                                 # neither
    st = L.GatStats(PTR, PTR, PTR, PTR)
    d = _desc(L, form="es")
    d.stats = ctypes.pointer(st)
    _refused(L, d, UNSUPPORTED)                          # both
    d = _desc(L, form=None)
    d.stats = ctypes.pointer(st)
    assert lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d)) > 0
    st_bad = L.GatStats(PTR, None, PTR, PTR)
    d.stats = ctypes.pointer(st_bad)
    _refused(L, d, NULL)                                 # a member of the statistics missing


def test_attention_grad_argument_errors(L):
    lib = L.lib
    need = lib.sgx_gat_attention_grad_workspace_bytes(1000, 16)
    assert need == (1000 + 63) // 64 * 2 * 16 * 4 and need % 256 == 0                   # the grid rule: a slice per 64 rows ...
    assert lib.sgx_gat_attention_grad_workspace_bytes(10 ** 6, 16) == 1024 * 2 * 16 * 4   # ... at most 1024
    assert lib.sgx_gat_attention_grad_workspace_bytes(0, 16) == 256                      # one slice, rounded up
    assert lib.sgx_gat_attention_grad_workspace_bytes(-1, 16) == 0 and lib.sgx_gat_attention_grad_workspace_bytes(5, 0) == 0
    ok = [1000, 1000, 16, PTR, PTR, PTR, PTR, PTR, 16, PTR, PTR, need, None]

    def call(**kw):
        names = ("n_rows", "n_cols", "n_feat", "rowPtr", "columnIndex", "sg", "g1", "Wh", "ldw", "out", "ws", "ws_bytes", "stream")
        a = [kw.get(n, v) for n, v in zip(names, ok)]
        return lib.sgx_gat_attention_grad(*a)

    assert call(n_rows=-1) == SHAPE and call(n_cols=999) == SHAPE and call(n_feat=0) == SHAPE and call(ldw=15) == SHAPE
    for name in ("rowPtr", "columnIndex", "sg", "g1", "Wh", "out"):
        assert call(**{name: None}) == NULL, name
    assert call(n_cols=2 ** 30, ldw=16) == UNSUPPORTED                                  # the table past 32-bit byte offsets
    assert call(ws=None) == WORKSPACE and call(ws_bytes=need - 1) == WORKSPACE
    assert call(ws=PTR + 64) == ALIGN
