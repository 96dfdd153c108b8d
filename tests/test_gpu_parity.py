"""Parity of the HIP path (through the C ABI) with the CPU oracle, on a real MI355X.

Tolerances (SURVEY 8c / BASELINE.md): fp16 storage + fp32 accumulation against exact math on
the same (half-rounded) inputs with H kept in fp16: atol 2e-3, rtol 1e-2 -- the band the
reference's own half kernel sits in; in practice the device lands ~10x tighter, which the
tests also assert where the summation order cannot matter.  fp32: rtol 1e-5 (scaled by the
row's |sum|).  CSR structure and helpers: bit exact.
"""
import numpy as np
import pytest
import torch

from _fixtures import SHAPES, half_ulp_distance, known_answers, load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sgx():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from sgracex1_amd import ops
    return ops


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t if dtype is None else t.to(dtype)


def _csr(sgx, csr, n_cols, dtype):
    rp, ci, va = csr
    return sgx.Csr(_dev(rp.astype(np.int32)), _dev(ci.astype(np.int32)), _dev(va.astype(np.float32), dtype), n_cols)


def _h(oracle, a):
    """round to half and back: the values the fp16 device path actually sees"""
    return oracle.to_half(np.asarray(a, np.float32)).astype(np.float32)


def _rand_csr(rng, n_rows, n_cols, avg_deg, empty_frac=0.2, long_rows=()):
    deg = rng.poisson(avg_deg, n_rows)
    deg[rng.random(n_rows) < empty_frac] = 0
    for r, d in long_rows:
        deg[r] = d
    deg = np.minimum(deg, n_cols)
    rp = np.zeros(n_rows + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = np.concatenate([np.sort(rng.choice(n_cols, d, replace=False)) for d in deg] + [np.zeros(0, np.int64)])
    va = rng.standard_normal(rp[-1]).astype(np.float32)
    return rp, ci.astype(np.int32), va


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["test", "test2", "mol", "cora", "citeseer"])
@pytest.mark.parametrize("relu", [0, 1])
def test_layer_fp16_reference_matrices(sgx, oracle, name, relu):
    d = load(name)
    adj_h = (d["adj"][0], d["adj"][1], _h(oracle, d["adj"][2]))
    fea_h = (d["fea"][0], d["fea"][1], _h(oracle, d["fea"][2]))
    Wt_h = _h(oracle, d["Wt"])
    want = oracle.layer_f64(0, relu, adj_h, fea_h, Wt_h, h_round=2)
    A = _csr(sgx, d["adj"], d["N"], torch.float16)
    X = _csr(sgx, d["fea"], d["M_fea"], torch.float16)
    got = sgx.layer_forward(A, X, _dev(d["Wt"], torch.float16), relu=relu)
    torch.cuda.synchronize()
    got = got.float().cpu().numpy()
    assert got.shape == (d["N"], d["P"])
    np.testing.assert_allclose(got, want, rtol=1e-2, atol=2e-3)
    # fp32 accumulation + one rounding: within 1 half ulp of the rounded exact value, except
    # where H's own rounding tips a tie; allow 2 ulp and require >= 99% exact
    ulp = half_ulp_distance(got.astype(np.float16), want.astype(np.float16))
    assert ulp.max() <= 2 and (ulp == 0).mean() > 0.99


def test_layer_known_answers_fp16(sgx, oracle):
    """The device path against the numbers the reference recorded (csim log / hardware row):
    its fp32-accumulated result must sit within 2e-3 of every logged half value."""
    d = load("citeseer")
    ka = known_answers()
    A = _csr(sgx, d["adj"], d["N"], torch.float16)
    X = _csr(sgx, d["fea"], d["M_fea"], torch.float16)
    got = sgx.layer_forward(A, X, _dev(d["Wt"], torch.float16), relu=0).float().cpu().numpy()
    for r in ("0", "31"):
        want = np.array([float(t) for t in ka["csim_log"][r]])
        np.testing.assert_allclose(got[int(r)], want, rtol=1e-2, atol=2e-3)
    hw = np.array([float(t) for t in ka["hw_row0_fp16_P16"]])
    np.testing.assert_allclose(got[0, :16], hw, rtol=1e-2, atol=2e-3)
    k = load("test")
    A = _csr(sgx, k["adj"], 4, torch.float16)
    X = _csr(sgx, k["fea"], 4, torch.float16)
    out = sgx.layer_forward(A, X, _dev(k["Wt"], torch.float16)).float().cpu().numpy()
    assert np.array_equal(out, np.array(ka["test_kat"]["D"], np.float32))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_layer_dense_features_mol(sgx, oracle, dtype):
    """gemm_mode 1 (dense X on the matrix cores) == gemm_mode 0 on the one-hot mol features."""
    d = load("mol")
    rnd = (lambda a: _h(oracle, a)) if dtype == torch.float16 else (lambda a: np.asarray(a, np.float32))
    want = oracle.layer_f64(1, 1, (d["adj"][0], d["adj"][1], rnd(d["adj"][2])), rnd(d["fea_dense"]), rnd(d["Wt"]),
                            h_round=2 if dtype == torch.float16 else 1)
    A = _csr(sgx, d["adj"], d["N"], dtype)
    Wt = _dev(d["Wt"], dtype)
    dense = sgx.layer_forward(A, _dev(d["fea_dense"], dtype), Wt, relu=1)
    sparse = sgx.layer_forward(A, _csr(sgx, d["fea"], d["M_fea"], dtype), Wt, relu=1)
    assert torch.equal(dense, sparse)               # one nonzero per row: both orders are exact
    tol = dict(rtol=1e-2, atol=2e-3) if dtype == torch.float16 else dict(rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dense.float().cpu().numpy(), want, **tol)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("P", [1, 2, 7, 8, 21, 24, 64, 100, 128, 256, 520])
def test_spmm_ragged_shapes(sgx, oracle, dtype, P):
    """Empty rows, a row count that is not a multiple of the rows per wavefront, every lane
    grouping (LPR 1..64), the scalar path (odd P) and the column-tile loop (P > 512)."""
    rng = np.random.default_rng(P)
    n_rows, n_cols = 1003, 777
    rp, ci, va = _rand_csr(rng, n_rows, n_cols, 9.0)
    H = rng.standard_normal((n_cols, P)).astype(np.float32)
    if dtype == torch.float16:
        va, H = _h(oracle, va), _h(oracle, H)
    want = oracle.spmm_f32(1, (rp, ci, va), H.astype(np.float64).astype(np.float32))
    exact = np.maximum(_dense(rp, ci, va, n_rows, n_cols).astype(np.float64) @ H.astype(np.float64), 0)
    A = _csr(sgx, (rp, ci, va), n_cols, dtype)
    got = sgx.spmm(A, _dev(H, dtype), relu=True).float().cpu().numpy()
    assert not got[np.diff(rp) == 0].any()                          # empty rows are exactly +0
    scale = np.abs(_dense(rp, ci, np.abs(va), n_rows, n_cols)) @ np.abs(H) + 1e-30
    if dtype == torch.float16:
        np.testing.assert_allclose(got, exact, rtol=2e-3, atol=2e-3)
    else:
        assert (np.abs(got - exact) / scale).max() < 1e-5
    np.testing.assert_allclose(got, want, rtol=1e-2, atol=2e-3)


def _dense(rp, ci, va, n_rows, n_cols):
    out = np.zeros((n_rows, n_cols), np.float32)
    rows = np.repeat(np.arange(n_rows), np.diff(rp))
    np.add.at(out, (rows, ci), va)
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_spmm_long_rows_split_path(sgx, oracle, dtype):
    """Rows longer than the plan's threshold are summed by several wavefronts; with and
    without a plan the results agree to rounding and both match the exact sum."""
    rng = np.random.default_rng(7)
    n_rows, n_cols, P = 300, 6000, 64
    rp, ci, va = _rand_csr(rng, n_rows, n_cols, 6.0, long_rows=[(0, 513), (17, 5000), (299, 1500), (150, 512)])
    va *= 0.05
    H = rng.standard_normal((n_cols, P)).astype(np.float32)
    if dtype == torch.float16:
        va, H = _h(oracle, va), _h(oracle, H)
    exact = _dense(rp, ci, va, n_rows, n_cols).astype(np.float64) @ H.astype(np.float64)
    A = _csr(sgx, (rp, ci, va), n_cols, dtype)
    # a small matrix (< 2^20 entries): rows over 64 edges are cut into 64-edge tasks (large ones: 512)
    assert A.plan.long_threshold == 64 and A.plan.long_rows == 4
    with_plan = sgx.spmm(A, _dev(H, dtype), relu=False, use_plan=True).float().cpu().numpy()
    no_plan = sgx.spmm(A, _dev(H, dtype), relu=False, use_plan=False).float().cpu().numpy()
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(with_plan, exact, **tol)
    np.testing.assert_allclose(no_plan, exact, **tol)
    short = np.diff(rp) <= A.plan.long_threshold
    assert np.array_equal(with_plan[short], no_plan[short])         # untouched rows: same kernel, same bits
    again = sgx.spmm(A, _dev(H, dtype), relu=False, use_plan=True).float().cpu().numpy()
    assert np.array_equal(with_plan, again)                         # split sums are order-fixed


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("M,P", [(7, 64), (64, 64), (100, 256), (602, 128), (33, 21), (64, 7), (1433, 16), (40, 300),
                                 (128, 128), (200, 48), (256, 24)])
@pytest.mark.parametrize("n", [1037, 9001])
def test_xw_dense_mfma(sgx, oracle, dtype, M, P, n):
    """n = 1037 runs the tiled kernel, n = 9001 (fp16, M <= 640) the weights-stationary one."""
    rng = np.random.default_rng(M * 1000 + P)
    X = rng.standard_normal((n, M)).astype(np.float32)
    W = (rng.standard_normal((M, P)) / np.sqrt(M)).astype(np.float32)
    if dtype == torch.float16:
        X, W = _h(oracle, X), _h(oracle, W)
    exact = X.astype(np.float64) @ W.astype(np.float64)
    got = sgx.xw_dense(_dev(X, dtype), _dev(np.ascontiguousarray(W.T), dtype))
    assert got.shape == (n, P)
    got = got.float().cpu().numpy()
    if dtype == torch.float16:
        np.testing.assert_allclose(got, exact, rtol=2e-3, atol=2e-3)
        # one rounding of an fp32 sum: off by more than 1 half ulp only where the terms cancel
        scale = np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64)
        ulp = half_ulp_distance(got.astype(np.float16), exact.astype(np.float16))
        assert (ulp <= 1).mean() > 0.999 and (np.abs(got - exact) <= 1e-3 * scale + 1e-6).all()
    else:
        scale = np.abs(X).astype(np.float64) @ np.abs(W).astype(np.float64)
        assert (np.abs(got - exact) / scale).max() < 2e-6


def test_xw_dense_pad_columns_are_zero(sgx):
    X = torch.randn(100, 64, device="cuda", dtype=torch.float16)
    Wt = torch.randn(21, 64, device="cuda", dtype=torch.float16)
    H = sgx.xw_dense(X, Wt, ldh=24)
    base = H.as_strided((100, 24), (24, 1))
    assert not base[:, 21:].any()


@pytest.mark.parametrize("name", ["cora", "citeseer"])
def test_two_layer_forward_fp16(sgx, oracle, name):
    """Layer 1 sparse X + ReLU, layer 2 dense X (the molecule_gcn / paper configuration)."""
    d = load(name)
    g = np.load(__import__("os").path.join(__import__("_fixtures").GOLD, name + ".npz"))
    W2 = g["w2"].astype(np.float32)
    adj_h = (d["adj"][0], d["adj"][1], _h(oracle, d["adj"][2]))
    fea_h = (d["fea"][0], d["fea"][1], _h(oracle, d["fea"][2]))
    l1 = oracle.layer_f64(0, 1, adj_h, fea_h, _h(oracle, d["Wt"]), h_round=2)
    l1h = _h(oracle, l1)
    l2 = oracle.layer_f64(1, 0, adj_h, l1h, _h(oracle, np.ascontiguousarray(W2.T)), h_round=2)
    A = _csr(sgx, d["adj"], d["N"], torch.float16)
    X = _csr(sgx, d["fea"], d["M_fea"], torch.float16)
    o1 = sgx.layer_forward(A, X, _dev(d["Wt"], torch.float16), relu=1)
    o2 = sgx.layer_forward(A, o1, _dev(np.ascontiguousarray(W2.T), torch.float16), relu=0)
    np.testing.assert_allclose(o2.float().cpu().numpy(), l2, rtol=1e-2, atol=2e-3)


def test_bias_count_quirk(sgx):
    """K.cpp:3876-3889: bias_count > 0 preloads and returns; D keeps its old contents."""
    d = load("mol")
    A = _csr(sgx, d["adj"], d["N"], torch.float16)
    X = _csr(sgx, d["fea"], d["M_fea"], torch.float16)
    out = torch.full((d["N"], d["P"]), 7.0, dtype=torch.float16, device="cuda")
    sgx.layer_forward(A, X, _dev(d["Wt"], torch.float16), out=out, bias_count=1)
    assert (out == 7).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("F", [8, 32, 64])
def test_gat_aggregate(sgx, oracle, dtype, F):
    rng = np.random.default_rng(F)
    n = 501
    rp, ci, va = _rand_csr(rng, n, n, 7.0, empty_frac=0.0)
    # self loops guarantee a positive edge per row, as sym_norm2 does (SG.py:42)
    dense = _dense(rp, ci, np.abs(va) + 0.1, n, n)
    dense[np.arange(n), np.arange(n)] = 1.0
    dense[rng.random((n, n)) < 0.002] = -0.5               # stored but masked out (adj > 0 test)
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    va = dense[rows, cols].astype(np.float32)
    Wh = rng.standard_normal((n, F)).astype(np.float32)
    att = (rng.standard_normal(2 * F) * 0.3).astype(np.float32)
    if dtype == torch.float16:
        va, Wh, att = _h(oracle, va), _h(oracle, Wh), _h(oracle, att)
    for relu in (0, 1):
        D, E, S = oracle.gat_f64(relu, (rp, cols.astype(np.int32), va), Wh, att, 0.2)
        A = _csr(sgx, (rp, cols.astype(np.int32), va), n, dtype)
        got, gE, gS = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att, dtype), alpha=0.2, relu=relu,
                                        want_edge_outputs=True)
        tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(got.float().cpu().numpy(), D, **tol)
        np.testing.assert_allclose(gE.cpu().numpy(), E, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(gS.cpu().numpy(), S, rtol=1e-4, atol=1e-6)
        assert (gS.cpu().numpy()[va <= 0] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("heads,f_head", [(8, 32), (4, 12), (2, 64), (3, 5)])
def test_gat_multi_head_is_the_single_head_formula_per_slice(sgx, oracle, dtype, heads, f_head):
    """n_heads > 1 = the reference's single-head formula on each column slice with its own attention
    vector (the oracle's gat_f64 per slice), concatenated; also against the kernel's own single-head runs."""
    rng = np.random.default_rng(heads * 100 + f_head)
    n, F = 403, heads * f_head
    rp, ci, va = _rand_csr(rng, n, n, 9.0, empty_frac=0.0)
    dense = _dense(rp, ci, np.abs(va) + 0.1, n, n)
    dense[np.arange(n), np.arange(n)] = 1.0
    dense[rng.random((n, n)) < 0.003] = -0.5
    dense[11, :] = 0                                         # a row without any edge
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    va = dense[rows, cols].astype(np.float32)
    Wh = rng.standard_normal((n, F)).astype(np.float32)
    att = (rng.standard_normal((heads, 2 * f_head)) * 0.3).astype(np.float32)
    if dtype == torch.float16:
        va, Wh, att = _h(oracle, va), _h(oracle, Wh), _h(oracle, att)
    csr = (rp, cols.astype(np.int32), va)
    A = _csr(sgx, csr, n, dtype)
    got, gE, gS = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=1, want_edge_outputs=True,
                                    heads=heads, fill_dead_rows=False)
    assert gE.shape == (len(va), heads) and gS.shape == (len(va), heads)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=2e-5, atol=2e-6)
    for h in range(heads):
        sl = slice(h * f_head, (h + 1) * f_head)
        D, E, S = oracle.gat_f64(1, csr, np.ascontiguousarray(Wh[:, sl]), att[h], 0.2)
        np.testing.assert_allclose(got[:, sl].float().cpu().numpy(), D, **tol)
        np.testing.assert_allclose(gE[:, h].cpu().numpy(), E, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(gS[:, h].cpu().numpy(), S, rtol=1e-4, atol=1e-6)
        one = sgx.gat_aggregate(A, _dev(np.ascontiguousarray(Wh[:, sl]), dtype), _dev(att[h], dtype), relu=1,
                                fill_dead_rows=False)
        np.testing.assert_allclose(got[:, sl].float().cpu().numpy(), one.float().cpu().numpy(), rtol=tol["rtol"],
                                   atol=max(tol["atol"], 1e-5))      # two fp32 orders of the same sums
    assert (got[11] == 0).all()
    # rows without a live edge, dense-emulation rule: the mean of all rows of Wh, per column
    filled = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=0, heads=heads)
    np.testing.assert_allclose(filled[11].float().cpu().numpy(), Wh.mean(0), **tol)
    # through the layer entry point: X = I makes X.W = Wh exactly
    X = torch.eye(n, dtype=dtype, device="cuda")
    out = sgx.layer_forward(A, X, _dev(np.ascontiguousarray(Wh.T), dtype), relu=1,
                            gat_attention=_dev(att.reshape(-1), dtype), gat_heads=heads)
    ref = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=1, heads=heads)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("F", [64, 256, 20])
def test_gat_long_rows_take_the_split_path(sgx, oracle, dtype, F):
    """Hub rows (> 512 edges) are cut into tasks with running softmax states merged in a fixed order:
    same result as the oracle and as the unsplit kernel, E / S included, a fully masked hub row too."""
    rng = np.random.default_rng(F)
    n = 3000
    rp, ci, va = _rand_csr(rng, n, n, 6.0, empty_frac=0.0)
    dense = _dense(rp, ci, np.abs(va) + 0.1, n, n)
    dense[np.arange(n), np.arange(n)] = 1.0
    for r, k, sign in ((5, 2500, 1.0), (77, 1200, 1.0), (1500, 800, -1.0), (2999, 513, 1.0)):
        cols = rng.choice(n, k, replace=False)
        dense[r, :] = 0
        dense[r, cols] = sign * (rng.random(k) + 0.05)
    dense[5, rng.choice(n, 300, replace=False)] *= -1                     # masked edges inside a hub row
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    va = dense[rows, cols].astype(np.float32)
    Wh = rng.standard_normal((n, F)).astype(np.float32)
    att = (rng.standard_normal(2 * F) * (0.6 / np.sqrt(F))).astype(np.float32)
    if dtype == torch.float16:
        va, Wh, att = _h(oracle, va), _h(oracle, Wh), _h(oracle, att)
    csr = (rp, cols.astype(np.int32), va)
    D, E, S = oracle.gat_f64(1, csr, Wh, att, 0.2)
    A = _csr(sgx, csr, n, dtype)
    assert A.plan.long_rows == 4
    got, gE, gS = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att, dtype), relu=1, want_edge_outputs=True,
                                    fill_dead_rows=False)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=3e-5, atol=3e-6)
    np.testing.assert_allclose(got.float().cpu().numpy(), D, **tol)
    np.testing.assert_allclose(gE.cpu().numpy(), E, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gS.cpu().numpy(), S, rtol=2e-4, atol=1e-7)
    assert (got[1500] == 0).all() and abs(float(gS[rp[5]:rp[6]].sum()) - 1.0) < 1e-4
    plain, pE, pS = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att, dtype), relu=1, want_edge_outputs=True,
                                      fill_dead_rows=False, use_plan=False)
    np.testing.assert_allclose(got.float().cpu().numpy(), plain.float().cpu().numpy(), **tol)
    assert torch.equal(gE, pE)
    # without the side outputs the one-walk form runs (csrc/gat_fused.hip): its own rounding, the same bits every run
    # (fixed merge order), and the two-stage form's bits when that is asked for
    again = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att, dtype), relu=1, fill_dead_rows=False)
    assert torch.equal(again, sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att, dtype), relu=1, fill_dead_rows=False))
    np.testing.assert_allclose(again.float().cpu().numpy(), D, **tol)
    assert (again[1500] == 0).all()
    from sgracex1_amd import _lib
    with _lib.tuning(SGX_GAT_FUSED="0"):
        assert torch.equal(sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att, dtype), relu=1, fill_dead_rows=False), got)
    filled = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att, dtype), relu=0)          # dense-emulation rule for the masked hub
    np.testing.assert_allclose(filled[1500].float().cpu().numpy(), Wh.mean(0), **tol)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("heads,f_head", [(8, 32), (4, 16), (3, 5)])
def test_gat_multi_head_long_rows(sgx, oracle, dtype, heads, f_head):
    """Several heads on a graph with hub rows: the plan's tasks leave per-head chunk states that are
    merged in task order -- against the oracle per column slice, and against the unsplit kernel."""
    rng = np.random.default_rng(heads + f_head)
    n, F = 2500, heads * f_head
    rp, ci, va = _rand_csr(rng, n, n, 5.0, empty_frac=0.0)
    dense = _dense(rp, ci, np.abs(va) + 0.1, n, n)
    dense[np.arange(n), np.arange(n)] = 1.0
    for r, k, sign in ((9, 2000, 1.0), (1200, 700, 1.0), (2400, 300, -1.0)):
        cols = rng.choice(n, k, replace=False)
        dense[r, :] = 0
        dense[r, cols] = sign * (rng.random(k) + 0.05)
    dense[9, rng.choice(n, 200, replace=False)] *= -1
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    va = dense[rows, cols].astype(np.float32)
    Wh = rng.standard_normal((n, F)).astype(np.float32)
    att = (rng.standard_normal((heads, 2 * f_head)) * (0.6 / np.sqrt(f_head))).astype(np.float32)
    if dtype == torch.float16:
        va, Wh, att = _h(oracle, va), _h(oracle, Wh), _h(oracle, att)
    csr = (rp, cols.astype(np.int32), va)
    A = _csr(sgx, csr, n, dtype)
    assert A.plan.long_rows == 3
    got, gE, gS = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=1, want_edge_outputs=True,
                                    heads=heads, fill_dead_rows=False)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=3e-5, atol=3e-6)
    for h in range(heads):
        sl = slice(h * f_head, (h + 1) * f_head)
        D, E, S = oracle.gat_f64(1, csr, np.ascontiguousarray(Wh[:, sl]), att[h], 0.2)
        np.testing.assert_allclose(got[:, sl].float().cpu().numpy(), D, **tol)
        np.testing.assert_allclose(gE[:, h].cpu().numpy(), E, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(gS[:, h].cpu().numpy(), S, rtol=2e-4, atol=1e-7)
    assert (got[2400] == 0).all()
    plain = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=1, heads=heads, fill_dead_rows=False,
                              use_plan=False)
    np.testing.assert_allclose(got.float().cpu().numpy(), plain.float().cpu().numpy(), rtol=tol["rtol"], atol=max(tol["atol"], 1e-5))
    again = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=1, heads=heads, fill_dead_rows=False)
    assert torch.equal(again, sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=1, heads=heads, fill_dead_rows=False))
    np.testing.assert_allclose(again.float().cpu().numpy(), got.float().cpu().numpy(), rtol=tol["rtol"], atol=max(tol["atol"], 1e-5))
    from sgracex1_amd import _lib
    with _lib.tuning(SGX_GAT_FUSED="0"):
        assert torch.equal(sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=1, heads=heads, fill_dead_rows=False), got)
    filled = sgx.gat_aggregate(A, _dev(Wh, dtype), _dev(att.reshape(-1), dtype), relu=0, heads=heads)
    np.testing.assert_allclose(filled[2400].float().cpu().numpy(), Wh.mean(0), **tol)


def test_gat_layer_through_desc(sgx, oracle):
    d = load("cora")
    rng = np.random.default_rng(3)
    att = (rng.standard_normal(2 * d["P"]) * 0.3).astype(np.float32)
    adj_h = (d["adj"][0], d["adj"][1], _h(oracle, d["adj"][2]))
    fea_h = (d["fea"][0], d["fea"][1], _h(oracle, d["fea"][2]))
    _, H = oracle.layer_f64(0, 0, adj_h, fea_h, _h(oracle, d["Wt"]), h_round=2, return_h=True)
    want, _, _ = oracle.gat_f64(1, adj_h, H, _h(oracle, att), 0.2)
    A = _csr(sgx, d["adj"], d["N"], torch.float16)
    X = _csr(sgx, d["fea"], d["M_fea"], torch.float16)
    got = sgx.layer_forward(A, X, _dev(d["Wt"], torch.float16), relu=1, gat_attention=_dev(att, torch.float16))
    np.testing.assert_allclose(got.float().cpu().numpy(), want, rtol=1e-2, atol=2e-3)


def test_helpers_bit_exact(sgx):
    rng = np.random.default_rng(11)
    # transpose with padded output
    x = torch.randn(37, 53, device="cuda", dtype=torch.float16)
    t = sgx.transpose(x, ldo=40)
    assert torch.equal(t[:, :37], x.t()) and not t[:, 37:].any()
    xf = torch.randn(64, 7, device="cuda")
    assert torch.equal(sgx.transpose(xf), xf.t().contiguous())
    # COO -> CSR, with empty rows at both ends
    n = 1000
    rows = np.sort(rng.integers(5, n - 5, 4000)).astype(np.int32)
    A = sgx.Csr.from_coo(_dev(rows), _dev(rng.integers(0, n, 4000).astype(np.int32)),
                         torch.ones(4000, device="cuda", dtype=torch.float16), n, n)
    want = np.zeros(n + 1, np.int64)
    want[1:] = np.cumsum(np.bincount(rows, minlength=n))
    assert np.array_equal(A.rowptr.cpu().numpy(), want)
    A.validate()
    # validation catches a broken structure
    bad = sgx.Csr(A.rowptr.clone(), A.col.clone(), A.val, n)
    bad.col[5] = n + 3
    with pytest.raises(RuntimeError):
        bad.validate()
    bad = sgx.Csr(A.rowptr.clone(), A.col, A.val, n)
    bad.rowptr[10] = bad.rowptr[11] + 1
    with pytest.raises(RuntimeError):
        bad.validate()
    # ReLU mask of RPYNQ.backward
    out = torch.tensor([0.0, 1.0, -0.0, 2.0], device="cuda", dtype=torch.float16)
    grad = torch.tensor([5.0, 6.0, 7.0, 8.0], device="cuda")
    sgx.relu_mask_backward_(out, grad)
    assert grad.tolist() == [0.0, 6.0, 0.0, 8.0]


def test_from_dense_matches_torch_csr(sgx):
    dense = (torch.rand(200, 200, device="cuda") < 0.03).float()
    A = sgx.Csr.from_dense(dense, torch.float16)
    sp = dense.to_sparse_csr()
    assert torch.equal(A.rowptr.long(), sp.crow_indices()) and torch.equal(A.col.long(), sp.col_indices())


def test_spmm_table_beyond_4gib(sgx):
    """A gathered table of 4 GiB or more (the all-gathered H of an 8-GPU run) takes the 64-bit
    pointer path instead of 32-bit buffer offsets; rows on both sides of the 4 GiB line."""
    n_cols, P = (1 << 25) + 4096, 64                                # 4.0005 GiB of fp16
    H = torch.empty((n_cols, P), dtype=torch.float16, device="cuda")
    H.copy_(((torch.arange(n_cols, device="cuda") % 251).to(torch.float16) / 16).unsqueeze(1).expand(n_cols, P))
    H[:, 1] = 1.0
    rng = np.random.default_rng(5)
    n_rows = 4099
    deg = rng.integers(0, 12, n_rows)
    rp = np.zeros(n_rows + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, n_cols, rp[-1]).astype(np.int32)
    ci[::3] = n_cols - 1 - (ci[::3] % 4096)                          # plenty of rows past 2^32 bytes
    va = (rng.integers(1, 5, rp[-1]) / 4).astype(np.float32)
    A = sgx.Csr(_dev(rp), _dev(ci), _dev(va, torch.float16), n_cols)
    got = sgx.spmm(A, H, relu=False, use_plan=False).float()
    rows = torch.as_tensor(np.repeat(np.arange(n_rows), deg), device="cuda")
    want = torch.zeros((n_rows, P), device="cuda").index_add_(0, rows, H[torch.as_tensor(ci, device="cuda").long()].float()
                                                            * torch.as_tensor(va, device="cuda").unsqueeze(1))
    assert torch.allclose(got, want, rtol=2e-3, atol=2e-3)
    assert torch.allclose(got[:, 1], torch.as_tensor(np.add.reduceat(np.append(va, 0), rp[:-1]) * (deg > 0),
                                                      device="cuda", dtype=torch.float32), rtol=2e-3, atol=2e-3)
    # empty slots of a lane group (degrees 1..7 fill 1..7 of its 8 slots) must not touch row 0 of the table: with a
    # non-finite H[0] every row that does not reference column 0 stays finite
    H[0] = float("inf")
    A1 = sgx.Csr(_dev(rp), _dev(np.maximum(ci, 1)), _dev(va, torch.float16), n_cols)
    assert (deg % 8 != 0).any() and torch.isfinite(sgx.spmm(A1, H, relu=False, use_plan=False).float()).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_pubmed_adjacency(sgx, oracle, dtype):
    """The reference's pubmed adjacency (19 717 nodes, 108 365 entries; GNN_arc.pdf Table 4 quotes pubmed) with its
    18 x 3 second-layer weights: the checkout holds no pubmed features (a missing large blob), so the case is the
    aggregation at the hidden width 18 over a seeded table, then the dense-X layer 18 -> 3 -- the narrowest output in
    the reference's data (one lane per row) -- against the exact-math oracle."""
    g = np.load(__import__("os").path.join(__import__("_fixtures").GOLD, "pubmed.npz"))
    rp, ci, va = g["adj_rowptr"], g["adj_col"], g["adj_val"]
    n = len(rp) - 1
    assert n == 19717 and len(ci) == 108365 and g["w"].shape == (500, 18) and g["w2"].shape == (18, 3)
    rng = np.random.default_rng(19717)
    H = rng.standard_normal((n, 18)).astype(np.float32)
    W2t = np.ascontiguousarray(g["w2"].T).astype(np.float32)
    if dtype == torch.float16:
        va, H, W2t = _h(oracle, va), _h(oracle, H), _h(oracle, W2t)
    A = _csr(sgx, (rp, ci, va), n, dtype)
    tol = dict(rtol=1e-2, atol=2e-3) if dtype == torch.float16 else dict(rtol=2e-5, atol=2e-5)
    D1 = sgx.spmm(A, _dev(H, dtype), relu=True)
    want1 = oracle.spmm_f32(1, (rp, ci, va), H)
    np.testing.assert_allclose(D1.float().cpu().numpy(), want1, **tol)
    D2 = sgx.layer_forward(A, D1, _dev(W2t, dtype), relu=False)
    assert D2.shape == (n, 3)
    want2 = oracle.layer_f64(1, 0, (rp, ci, va), D1.float().cpu().numpy(), W2t, h_round=2 if dtype == torch.float16 else 1)
    np.testing.assert_allclose(D2.float().cpu().numpy(), want2, **tol)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_two_pass_aggregation(sgx, dtype):
    """sgx_spmm_csr_acc: the edges split into two disjoint sets and aggregated in two passes (fp32
    partial in between) against the single pass, with long rows in both passes."""
    rng = np.random.default_rng(21)
    n_rows, n_cols, P = 2000, 3000, 64
    rp, ci, va = _rand_csr(rng, n_rows, n_cols, 12.0, long_rows=[(5, 1400), (900, 700)])
    va = (va * 0.1).astype(np.float32)
    H = torch.randn((n_cols, P), device="cuda").to(dtype)
    A = _csr(sgx, (rp, ci, va), n_cols, dtype)
    A.plan
    single = sgx.spmm(A, H, relu=True)
    first = ci < 1500                                                  # "own" columns / "halo" columns
    row = np.repeat(np.arange(n_rows), np.diff(rp))
    parts = []
    for m in (first, ~first):
        prp = np.zeros(n_rows + 1, np.int32)
        prp[1:] = np.cumsum(np.bincount(row[m], minlength=n_rows))
        B = _csr(sgx, (prp, ci[m], va[m]), n_cols, dtype)
        B.plan
        parts.append(B)
    partial = sgx.spmm_acc(parts[0], H, partial_out=True)
    assert partial.dtype == torch.float32
    two = sgx.spmm_acc(parts[1], H, relu=True, acc_in=partial)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=1e-4, atol=1e-5)
    assert torch.allclose(two.float(), single.float(), **tol)
    assert (two == single).float().mean() > 0.97


def test_fp16_subnormals_are_not_flushed(sgx):
    """Subnormal halves (|x| < 6.1e-5) in W, H and the adjacency values go through both gather loops
    (X.W with a CSR X uses v_fma_mix_f32, A.H converts and uses packed fmas) like any other value."""
    dev = torch.device("cuda")
    n, m, p = 257, 40, 64
    tiny = torch.tensor(2.0 ** -24, dtype=torch.float16)              # smallest positive half
    k = torch.arange(1, m * p + 1, dtype=torch.float32).reshape(p, m) % 23 + 1
    Wt = (k * float(tiny)).half().to(dev)                              # W entries: 1..23 units of 2^-24
    # X: two ones per row -> H[r] = W[c0] + W[c1] exactly (still subnormal or barely normal)
    c0 = torch.arange(n) % m
    c1 = (torch.arange(n) * 7 + 3) % m
    c1 = torch.where(c1 == c0, (c1 + 1) % m, c1)
    lo, hi = torch.minimum(c0, c1), torch.maximum(c0, c1)
    X = sgx.Csr(torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device=dev),
                torch.stack([lo, hi], 1).reshape(-1).to(torch.int32).to(dev), torch.ones(2 * n, dtype=torch.float16, device=dev), m)
    eye = sgx.Csr(torch.arange(n + 1, dtype=torch.int32, device=dev), torch.arange(n, dtype=torch.int32, device=dev),
                  torch.ones(n, dtype=torch.float16, device=dev), n)
    got = sgx.layer_forward(eye, X, Wt, relu=True)
    W = Wt.float().cpu().T                                              # [m, p]
    want = (W[lo] + W[hi]).half()
    assert (want > 0).all() and (want.float() < 6.2e-5).any()
    assert torch.equal(got.cpu(), want)
    # A.H with subnormal adjacency values and a subnormal table
    A = sgx.Csr(torch.arange(n + 1, dtype=torch.int32, device=dev), torch.arange(n, dtype=torch.int32, device=dev),
                torch.full((n,), 2.0 ** -12, dtype=torch.float16, device=dev), n)
    H = (torch.arange(1, n * p + 1, dtype=torch.float32).reshape(n, p) % 9 + 1) * 2.0 ** -12
    out = sgx.spmm(A, H.half().to(dev), relu=False)
    assert torch.equal(out.cpu(), (H * 2.0 ** -12).half()) and (out > 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("P", [64, 128, 24])
def test_sparse_features_with_very_short_rows(sgx, oracle, dtype, P):
    """X with ~3 entries per row and a row plan: the X.W stage runs with two 16-byte chunks per lane
    (CPL = 2, chosen below 5 entries per row) in its loads-first form -- against the exact-math oracle."""
    rng = np.random.default_rng(P)
    n, m = 40_000, 500
    deg = rng.integers(0, 7, n)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, m, rp[-1]).astype(np.int32)
    va = rng.standard_normal(rp[-1]).astype(np.float32)
    Wt = (rng.standard_normal((P, m)) * 0.1).astype(np.float32)
    if dtype == torch.float16:
        va, Wt = _h(oracle, va), _h(oracle, Wt)
    eye = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32))
    X = _csr(sgx, (rp, ci, va), m, dtype)
    assert X.nnz >= 8192 and X.nnz / n < 5 and X.wants_plan
    got = sgx.layer_forward(_csr(sgx, eye, n, dtype), X, _dev(Wt, dtype), relu=0)
    want = oracle.layer_f64(0, 0, eye, (rp, ci, va), Wt, h_round=2 if dtype == torch.float16 else 1)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(got.float().cpu().numpy(), want, **tol)
    assert not got[torch.as_tensor(deg == 0, device="cuda")].any()


@pytest.mark.parametrize("dtype,M,P", [(torch.float16, 300, 128), (torch.float16, 602, 256), (torch.float16, 256, 100),
                                       (torch.float32, 300, 128), (torch.float32, 200, 250)])
def test_xw_dense_tall_tiles(dtype, M, P):
    """Dense X.W with K > 128 on enough rows for the taller MFMA tiles (32 768 rows and more), ragged at the end:
    against the fp32 product of the same inputs, with and without the activation on the stores."""
    from sgracex1_amd import ops
    g = torch.Generator(device="cuda")
    g.manual_seed(M + P)
    n = 40_000 + 37
    X = (torch.rand((n, M), generator=g, device="cuda") - 0.4).to(dtype)
    Wt = ((torch.rand((P, M), generator=g, device="cuda") * 2 - 1) / M ** 0.5).to(dtype)
    want = X.float() @ Wt.float().t()
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float16 else dict(rtol=1e-5, atol=1e-5)
    got = ops.xw_dense(X, Wt)
    assert got.shape == (n, P) and torch.allclose(got.float(), want, **tol)
    act = ops.xw_dense(X, Wt, relu=True)
    assert torch.equal(act, torch.where(got > 0, got, torch.zeros_like(got)))
    # pad columns of the scratch pitch are exact zeros (the aggregation's vector gathers may read them)
    base = got._base if got._base is not None else got
    assert not base[:, P:].any()


@pytest.mark.parametrize("M,P", [(602, 128), (602, 256), (300, 128), (130, 16), (1000, 64), (2000, 40), (601, 128), (608, 41)])
def test_xw_dense_weights_in_lds(M, P):
    """Long K with all of W^T resident in LDS and X streamed through a register ring (xw_dense_wlds.hip) against the
    128 x 128 tile kernel it replaces: the same k-steps into the same MFMA in the same order, so the same bits -- one or
    two column blocks, 2 / 4 / 8 column tiles, K a multiple of 32 or not, odd K (2-byte aligned rows: stays with the
    tile kernel), a ragged last row tile.  Rows of NaN / Inf stay in their rows: a row's last k-step reads into the
    next row and is masked."""
    from sgracex1_amd import _lib, ops
    g = torch.Generator(device="cuda")
    g.manual_seed(M * 7 + P)
    n = 33_000 + 13
    X = (torch.rand((n, M), generator=g, device="cuda") - 0.4).half()
    Wt = ((torch.rand((P, M), generator=g, device="cuda") * 2 - 1) / M ** 0.5).half()
    bad = torch.tensor([1, 17, 4095, 20_000, n - 1], device="cuda")
    X[bad] = float("nan")
    X[bad + 0, 0] = float("inf")
    got = ops.xw_dense(X, Wt)
    act = ops.xw_dense(X, Wt, relu=True)
    with _lib.tuning(SGX_XW_NO_WLDS="1"):
        tile = ops.xw_dense(X, Wt)
    ok = torch.ones(n, dtype=torch.bool, device="cuda")
    ok[bad] = False
    assert torch.equal(got[ok], tile[ok]) and torch.isfinite(got[ok].float()).all()
    assert torch.isnan(got[~ok].float()).all()
    want = X[ok].float() @ Wt.float().t()
    torch.testing.assert_close(got[ok].float(), want, rtol=2e-3, atol=2e-3)
    assert torch.equal(act[ok], torch.where(got[ok] > 0, got[ok], torch.zeros_like(got[ok])))
    base = got._base if got._base is not None else got
    assert not base[ok][:, P:].any()


@pytest.mark.parametrize("dtype,F", [(torch.float16, 128), (torch.float16, 256), (torch.float16, 250), (torch.float32, 100),
                                     (torch.float32, 256)])
def test_gat_wide_rows_low_degree(oracle, dtype, F):
    """Wide Wh rows over a low-degree graph (a piece of 16-32 edges is mostly empty), masked edges among the stored
    ones: against the oracle (rows, E, S), and with / without the plan."""
    from sgracex1_amd import graphs, ops
    n = 6000
    A = graphs.uniform_graph(n, 36_000, seed=F, dtype=dtype)               # ~7 edges per row with the self loops
    assert A.wants_plan and 2 * A.nnz <= 16 * n
    g = torch.Generator(device="cuda")
    g.manual_seed(F)
    Wh = (torch.randn((n, F), generator=g, device="cuda") * 0.5).to(dtype)
    att = (torch.randn(2 * F, generator=g, device="cuda") * (0.5 / F ** 0.5)).to(dtype)
    A.val[::7] = -A.val[::7].abs()                                          # stored but masked edges
    got, E, S = ops.gat_aggregate(A, Wh, att, relu=True, want_edge_outputs=True)
    csr = (A.rowptr.cpu().numpy(), A.col.cpu().numpy(), A.val.float().cpu().numpy())
    want, wE, wS = oracle.gat_f64(1, csr, Wh.float().cpu().numpy(), att.float().cpu().numpy(), 0.2)
    live = torch.zeros(n, dtype=torch.bool, device="cuda")
    deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), deg)
    live[row[A.val > 0]] = True
    lv = live.cpu().numpy()
    tol = dict(rtol=1e-2, atol=2e-3) if dtype == torch.float16 else dict(rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(got.float().cpu().numpy()[lv], want[lv], **tol)
    np.testing.assert_allclose(S.cpu().numpy()[(lv[row.cpu().numpy()])], wS[lv[row.cpu().numpy()]], rtol=4e-3, atol=1e-5)
    np.testing.assert_allclose(E.cpu().numpy(), wE, rtol=2e-3, atol=2e-3)
    one_chunk = ops.gat_aggregate(A, Wh, att, relu=True, use_plan=False)
    assert torch.allclose(got.float(), one_chunk.float(), rtol=2e-3 if dtype == torch.float16 else 1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype,heads,F", [(torch.float16, 1, 256), (torch.float16, 8, 256), (torch.float16, 1, 64), (torch.float16, 4, 128),
                                           (torch.float32, 1, 64), (torch.float32, 8, 256), (torch.float16, 3, 96)])
@pytest.mark.parametrize("gen_name", ["uniform", "rmat"])
def test_gat_two_stage_with_and_without_edge_outputs(oracle, dtype, heads, F, gen_name):
    """The two-stage GAT aggregate with and without the E / S side outputs (the weights land in the caller's S or in
    scratch): the same rows bit for bit -- short rows, rows taken by a whole wavefront, hub rows cut into tasks, masked
    edges, rows without a live edge (R-MAT without self loops leaves thousands of empty rows) -- and inside the band of
    the oracle."""
    from sgracex1_amd import graphs, ops
    n = 40_000
    A = (graphs.rmat_graph_n if gen_name == "rmat" else graphs.uniform_graph)(n, 1_300_000, seed=F + heads, dtype=dtype,
                                                                               self_loops=(gen_name == "uniform"))
    g = torch.Generator(device="cuda")
    g.manual_seed(heads * 1000 + F)
    val = A.val.float()
    val[torch.rand(A.nnz, generator=g, device="cuda") < 0.02] = -0.25          # stored, masked out
    A = ops.Csr(A.rowptr, A.col, val.to(dtype), A.n_cols)
    if gen_name == "rmat":
        assert A.gat_plan.long_rows > 0 and int((A.rowptr[1:] == A.rowptr[:-1]).sum()) > 0
    Wh = (torch.randn((n, F), generator=g, device="cuda") * 0.5).to(dtype)
    att = (torch.randn(heads * 2 * (F // heads), generator=g, device="cuda") * (0.5 / (F // heads) ** 0.5)).to(dtype)
    junk = torch.full((20_000_000,), float("nan"), device="cuda")              # what the allocator hands out next is not zeros
    del junk
    from sgracex1_amd import _lib
    with _lib.tuning(SGX_GAT_FUSED="0"):          # (without side outputs the default is the one-walk form: tests/test_gpu_gat_fused.py)
        fly = ops.gat_aggregate(A, Wh, att, alpha=0.2, relu=True, heads=heads)
    with_edges, _E, S = ops.gat_aggregate(A, Wh, att, alpha=0.2, relu=True, heads=heads, want_edge_outputs=True)
    assert torch.equal(fly, with_edges)
    # rows without a live edge receive the mean row of Wh (the dense emulation's rule, SG.py:638-641) -- every one of
    # them, whichever kernel of stage A met it (a wavefront of empty rows once left their flags unwritten)
    deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), deg)
    live = torch.zeros(n, dtype=torch.int64, device="cuda").index_add_(0, row, (A.val.float() > 0).long()) > 0
    if (~live).any():
        mean_row = torch.relu(Wh.float().mean(0))
        for got in (fly, with_edges):
            torch.testing.assert_close(got[~live].float(), mean_row.expand(int((~live).sum()), F), rtol=1e-2, atol=2e-3)
    if heads == 1:
        csr = (A.rowptr.cpu().numpy(), A.col.cpu().numpy(), A.val.float().cpu().numpy())
        want, _wE, wS = oracle.gat_f64(1, csr, Wh.float().cpu().numpy(), att.float().cpu().numpy(), 0.2)
        tol = dict(rtol=1e-2, atol=2e-3) if dtype == torch.float16 else dict(rtol=2e-4, atol=2e-5)
        # rows with a live edge (the stored-edge oracle does not restate the dead-row rule)
        lv = live.cpu().numpy()
        np.testing.assert_allclose(fly.float().cpu().numpy()[lv], want[lv], **tol)
        np.testing.assert_allclose(S.cpu().numpy()[lv[row.cpu().numpy()]], wS[lv[row.cpu().numpy()]], rtol=4e-3, atol=1e-5)


@pytest.mark.parametrize("M,P", [(128, 256), (100, 47), (64, 64), (7, 21), (33, 300), (16, 16), (128, 8)])
def test_xw_dense_fp32_weights_in_registers(M, P):
    """fp32 X.W with K <= 128 on 8 K rows and more: the weights-stationary kernel (W fragments in registers, X streamed)
    against the tile kernel it replaces -- same sums in the same order, so the same bits -- and against torch in fp32;
    with the ReLU on the stores; ragged last tile, pad columns zero."""
    from sgracex1_amd import _lib, ops
    g = torch.Generator(device="cuda")
    g.manual_seed(M * 13 + P)
    n = 20_000 + 11
    X = torch.rand((n, M), generator=g, device="cuda") - 0.4
    Wt = (torch.rand((P, M), generator=g, device="cuda") * 2 - 1) / M ** 0.5
    got = ops.xw_dense(X, Wt)
    act = ops.xw_dense(X, Wt, relu=True)
    with _lib.tuning(SGX_XW_NO_STATIONARY_F32="1"):
        tile = ops.xw_dense(X, Wt)
    assert torch.equal(got, tile)
    torch.testing.assert_close(got, X @ Wt.t(), rtol=1e-5, atol=1e-5)
    assert torch.equal(act, torch.where(got > 0, got, torch.zeros_like(got)))
    base = got._base if got._base is not None else got
    assert not base[:, P:].any()


@pytest.mark.parametrize("M,P", [(128, 256), (100, 250), (48, 128), (128, 65), (64, 256), (33, 129), (128, 602), (64, 300), (128, 770)])
def test_xw_dense_fp32_weights_in_lds(M, P):
    """fp32 X.W, K <= 128, more than 64 output columns, 32 K rows and more: all of W^T in LDS and every wavefront on all
    column tiles of its row tiles (xw_dense_wlds_f32_kernel) against the tile kernel -- the same sums in the same order,
    the same bits -- against torch, with the ReLU on the stores, rows of NaN staying in their rows."""
    from sgracex1_amd import _lib, ops
    g = torch.Generator(device="cuda")
    g.manual_seed(M * 17 + P)
    n = 40_000 + 5
    X = torch.rand((n, M), generator=g, device="cuda") - 0.4
    Wt = (torch.rand((P, M), generator=g, device="cuda") * 2 - 1) / M ** 0.5
    bad = torch.tensor([0, 15, 16, 31_999, n - 1], device="cuda")
    X[bad] = float("nan")
    got = ops.xw_dense(X, Wt)
    act = ops.xw_dense(X, Wt, relu=True)
    with _lib.tuning(SGX_XW_NO_WLDS="1", SGX_XW_NO_STATIONARY_F32="1"):
        tile = ops.xw_dense(X, Wt)
    ok = torch.ones(n, dtype=torch.bool, device="cuda")
    ok[bad] = False
    assert torch.equal(got[ok], tile[ok]) and torch.isnan(got[~ok]).all()
    torch.testing.assert_close(got[ok], X[ok] @ Wt.t(), rtol=1e-5, atol=1e-5)
    assert torch.equal(act[ok], torch.where(got[ok] > 0, got[ok], torch.zeros_like(got[ok])))
    base = got._base if got._base is not None else got
    assert not base[ok][:, P:].any()


# the cases of the test below whose SC launch walks more than one row tile per wavefront, and their rows: the SC launches
# take the grid of the plain stationary <4, 4> launch at the same shape (stationary_waves, csrc/xw_dense.hip), whose form
# ops.xw_dense_form reports -- 2048 streams of 4 column groups walk 2049 row tiles, 1024 streams of 8 groups 1025
_SCORES_PAST_ONE_TRIP = {(96, 256, 8): 65_536 + 7, (100, 512, 1): 32_768 + 7}


@pytest.mark.parametrize("M,P,heads", [(128, 256, 8), (100, 256, 8), (64, 128, 4), (40, 64, 2), (128, 256, 1), (100, 256, 2),
                                       (64, 128, 1), (33, 64, 1), (128, 512, 1), *_SCORES_PAST_ONE_TRIP])
@pytest.mark.parametrize("gen_name", ["uniform", "rmat"])
def test_gat_layer_scores_from_the_product_epilogue(M, P, heads, gen_name):
    """A GAT layer whose heads are 32 columns or whole 64-column groups (one head of 256: the reference's semantics; 8 of
    32: BASELINE's configuration 5): the X.W kernel forms the attention scores beside H (SC forms of the stationary kernel;
    wide heads as a partial per 64-column group, added by a small kernel in the scores kernel's tree order) instead of a
    pass over H of its own.  Same eight-term chains and the same tree, so the layer equals -- bit for bit -- the same layer
    with SGX_GAT_NO_FUSED_SCORES and the composition xw_dense + gat_aggregate; E and S too."""
    from sgracex1_amd import _lib, graphs, ops
    n = _SCORES_PAST_ONE_TRIP.get((M, P, heads), 24_000 + 7)
    A = (graphs.rmat_graph_n if gen_name == "rmat" else graphs.uniform_graph)(n, 400_000, seed=M + P)
    g = torch.Generator(device="cuda")
    g.manual_seed(M * 3 + P)
    X = (torch.rand((n, M), generator=g, device="cuda") - 0.4).half()
    Wt = ((torch.rand((P, M), generator=g, device="cuda") * 2 - 1) / M ** 0.5).half()
    att = ((torch.rand(2 * P, generator=g, device="cuda") * 2 - 1) * 0.3).half()
    if (M, P, heads) in _SCORES_PAST_ONE_TRIP:
        form = ops.xw_dense_form(X, Wt)
        assert form[:3] == ("stationary", 4, 4) and form.blocks == P // 64 and form.max_trips >= 2 and n % 32 != 0, form
    fused, E, S = ops.layer_forward(A, X, Wt, relu=True, gat_attention=att, gat_heads=heads, want_edge_outputs=True)
    with _lib.tuning(SGX_GAT_NO_FUSED_SCORES="1"):
        plain, E0, S0 = ops.layer_forward(A, X, Wt, relu=True, gat_attention=att, gat_heads=heads, want_edge_outputs=True)
    assert torch.equal(fused, plain) and torch.equal(E, E0) and torch.equal(S, S0)
    Wh = ops.xw_dense(X, Wt)
    with _lib.tuning(SGX_GAT_FUSED="0"):
        composed = ops.gat_aggregate(A, Wh, att, alpha=0.2, relu=True, heads=heads)
    assert torch.equal(fused, composed)
    assert torch.isfinite(fused.float()).all()
    # without side outputs the aggregate may be the one-walk form (csrc/gat_fused.hip), which takes s1 from the same place:
    # the layer and the composition agree bit for bit there too
    assert torch.equal(ops.layer_forward(A, X, Wt, relu=True, gat_attention=att, gat_heads=heads),
                       ops.gat_aggregate(A, Wh, att, alpha=0.2, relu=True, heads=heads))
