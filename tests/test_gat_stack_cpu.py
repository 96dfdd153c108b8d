"""sgx_gat_stack_forward without a GPU: symbols, struct layout, argument errors, and the float64 restatement and batch the
GPU tests use (tests/_gat_stack_ref.py) checked for what they claim."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _gat_ref as R
import _gat_stack_ref as S
from _stack_ref import stack_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sgx_gat_stack_workspace_bytes", "sgx_gat_stack_forward"]
WIDTHS = [(7, 1), (7, 3), (64, 64), (7, 256), (64, 256)]          # (M_fea, P) of the GPU test's first layers


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_new_symbols_are_exported(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in NEW:
        assert name in L.SYMBOLS
        assert f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110


def test_gat_stack_structs_match_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof_layer %zu\\n", sizeof(sgx_gat_stack_layer));\n'
        ' printf("sizeof_desc %zu\\n", sizeof(sgx_gat_stack_desc));\n'
        + "".join(f' printf("l.{n} %zu\\n", offsetof(sgx_gat_stack_layer, {n}));\n' for n, _ in L.GatStackLayer._fields_)
        + "".join(f' printf("d.{n} %zu\\n", offsetof(sgx_gat_stack_desc, {n}));\n' for n, _ in L.GatStackDesc._fields_)
        + " return SGX_VERSION == 110 ? 0 : 1;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        seen += 1
        if name == "sizeof_layer":
            assert ctypes.sizeof(L.GatStackLayer) == int(val)
        elif name == "sizeof_desc":
            assert ctypes.sizeof(L.GatStackDesc) == int(val)
        elif name.startswith("l."):
            assert getattr(L.GatStackLayer, name[2:]).offset == int(val), name
        else:
            assert getattr(L.GatStackDesc, name[2:]).offset == int(val), name
    assert seen == 2 + len(L.GatStackLayer._fields_) + len(L.GatStackDesc._fields_)
    # the GCN descriptor's fields lie where they lie in sgx_stack_desc up to the layer array
    for n, _ in L.StackDesc._fields_[:L.StackDesc._fields_.index(("layer", L.StackLayer * 4)) + 1]:
        assert getattr(L.GatStackDesc, n).offset == getattr(L.StackDesc, n).offset


def _desc(L, n_layers=2):
    d = L.GatStackDesc()
    d.dtype, d.n_layers = 0, n_layers
    for l in range(4):
        d.layer[l].gemm_mode, d.layer[l].M_fea, d.layer[l].P_w = 1, 8, 8
    return d


def test_argument_errors_need_no_gpu(L):
    """Every pointer is NULL or a made-up address: nothing may be launched."""
    lib = L.lib
    fwd = lambda d: lib.sgx_gat_stack_forward(ctypes.byref(d), None)
    assert lib.sgx_gat_stack_forward(None, None) == -1                      # SGX_ERR_NULL
    assert lib.sgx_gat_stack_workspace_bytes(None) == 0
    for n in (0, 5):
        assert fwd(_desc(L, n)) == -2                                        # SGX_ERR_SHAPE
    d = _desc(L)
    assert fwd(d) == -1                                                      # no plan
    d.dtype = 7
    assert fwd(d) == -3
    h = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create(0, 0, 0, None, None, None, 64, ctypes.byref(h), None) == 0 and h.value
    try:
        d = _desc(L)
        d.plan = h
        d.n_graphs = 1
        assert fwd(d) == -2                                                  # graph count not the plan's
        d.n_graphs = 0
        assert fwd(d) == -1                                                  # B missing
        for l in range(2):
            d.layer[l].B = 256
        assert fwd(d) == 0 and lib.sgx_gat_stack_workspace_bytes(ctypes.byref(d)) == 0    # all GCN, nothing to do
        d.layer[1].gat_mode = 1
        assert fwd(d) == -1                                                  # attention NULL on a GAT layer
        assert lib.sgx_gat_stack_workspace_bytes(ctypes.byref(d)) == 0      # (a bad descriptor)
        d.layer[1].attention = 512
        assert fwd(d) == 0
        d.layer[0].attention = 0                                             # ... but not needed on a GCN layer
        assert fwd(d) == 0
        for bad in (2, -1):
            d.layer[0].gat_mode = bad
            assert fwd(d) == -3                                              # SGX_ERR_UNSUPPORTED
        d.layer[0].gat_mode = 0
        d.layer[2].gat_mode = 9                                              # past n_layers: not looked at
        assert fwd(d) == 0
        d.layer[1].M_fea = 9                                                 # the GCN call's errors stay
        assert fwd(d) == -2
        d.layer[1].M_fea, d.layer[1].gemm_mode = 8, 0
        assert fwd(d) == -3
        d.layer[1].gemm_mode, d.C = 1, 2
        assert fwd(d) == -1
    finally:
        assert lib.sgx_batch_plan_destroy(h) == 0


def test_row_budget_helper_is_the_library_s(L):
    lib = L.lib
    for dt, code in (("f16", 0), ("f32", 1)):
        for width in (1, 3, 7, 64, 100, 252, 256):
            for kind in (0, 1):
                h = ctypes.c_void_p()
                assert lib.sgx_batch_plan_create_ex(code, 0, 0, None, None, None, width, kind, ctypes.byref(h), None) == 0
                try:
                    assert lib.sgx_batch_plan_rows(h) == S.rows_budget(dt, width, backward=bool(kind)), (dt, width, kind)
                finally:
                    lib.sgx_batch_plan_destroy(h)
    assert S.rows_budget("f32", 252) == 32 and 2 * 32 * (252 + 4) * 4 == 65536     # the tiles that fill 64 KiB


def test_all_gcn_restatement_is_stack_f64():
    b = S.build_batch("f32", 64, 7, seed=3)
    rng = np.random.default_rng(0)
    Ws = [rng.standard_normal((7, 5)), rng.standard_normal((5, 9)), rng.standard_normal((9, 4))]
    hw, hb = rng.standard_normal((3, 4)), rng.standard_normal(3)
    adj = (b["rowptr"], b["col"], b["val"])
    got = S.chain_f64(adj, b["x"], Ws, [None] * 3, [True, False, True], b["graph_ptr"], hw, hb)
    outs, pooled, logits = stack_f64(adj, b["x"], Ws, [True, False, True], b["graph_ptr"], hw, hb)
    for a, w in zip(got["outs"], outs):
        np.testing.assert_allclose(a, w, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(got["pooled"], pooled, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(got["logits"], logits, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("m_in,P", WIDTHS)
def test_the_batch_holds_what_it_claims(L, dt, m_in, P):
    budget = S.rows_budget(dt, max(P, m_in))
    b = S.build_batch(dt, budget, m_in, seed=P)
    sizes = b["sizes"]
    assert 12 <= len(sizes) <= 20 and max(sizes) == budget and budget in sizes and 0 in sizes
    for n in (1, 2, 15, 16, 17):
        assert min(n, budget) in sizes
    assert b["graph_ptr"][-1] == b["n_rows"] and (np.diff(b["graph_ptr"]) == sizes).all()
    # block-diagonal: every stored entry stays in its row's graph
    g_of = np.repeat(np.arange(len(sizes)), sizes)
    assert (g_of[R.rows_of(b["rowptr"])] == g_of[b["col"]]).all()
    # at least 3 groups, counted by the library's own host-side rule
    groups = L.lib.sgx_batch_plan_group_count(0 if dt == "f16" else 1, b["n_rows"], max(sizes), max(P, m_in), 0)
    assert groups >= 3
    # from the float64 result alone
    W, att = S.first_layer(dt, m_in, P, seed=P)
    res = S.chain_f64((b["rowptr"], b["col"], b["val"]), b["x"], [W], [att], [False], b["graph_ptr"], dt=dt)
    r = res["refs"][0]
    row_of = {n: i for i, n in b["names"].items()}
    dead = {row_of["no_stored_entry"], row_of["all_masked_plus0_minus0_negative"]}
    assert dead <= set(np.nonzero(r["dead"])[0]) and (res["outs"][0][sorted(dead)] == 0).all()
    rp = b["rowptr"]

    def ents(name):
        i = row_of[name]
        return slice(rp[i], rp[i + 1])
    e = ents("one_live_among_masked")
    assert r["live"][e].sum() == 1 and (~r["live"][e]).sum() >= 2 and np.isclose(r["S"][e].sum(), 1.0)
    e = ents("max_on_last_entry")
    assert r["live"][e].all() and np.argmax(r["E"][e]) == e.stop - e.start - 1
    for name in ("spread_240_underflows", "spread_144_through_leaky"):
        e = ents(name)
        x = r["E"][e][r["live"][e]]
        assert x.max() - x.min() >= 104, (name, x)
        assert r["S"][e].min() < 2.0 ** -149                       # below fp32's smallest subnormal: it underflows
    e = ents("live_f16_subnormal")
    k = int(np.argmax(b["val"][e] == R.F16_SUB))
    assert b["val"][e][k] == R.F16_SUB and r["live"][e][k] and r["S"][e][k] > 0.99
    e = ents("masked_max")
    assert not r["live"][e][np.argmax(r["E"][e])]
    # the bounds are finite and small against the values
    assert np.isfinite(res["b_outs"][0]).all() and np.isfinite(res["b_pooled"]).all()
