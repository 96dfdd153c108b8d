"""tests/_refhalf_ref.py, the numpy float16 restatement of SGX_ACC_REF_HALF, against the oracle's model of the same mode
(oracle.layer_refhalf, itself tied to the csim log by test_oracle_pinned.py): bit for bit on every input and every
(spmm_block, fea_threads, adj_threads) that tests/test_gpu_refhalf_arms.py runs on the device.  Then the inputs themselves:
each piece of the arithmetic, when replaced, moves more than 1 % of the outputs, the hostile rows hold what their names say,
and every phase occurs."""
import numpy as np
import pytest

import _refhalf_ref as R


def _same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


def _eye_csr(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float16)


def test_first_row_splits():
    """1101 rows over 4 threads: blocks of 275, the last thread rows 825..1100; sblocks restart at 0, 275, 550, 825 and
    row 1100 (1100 // 275 = 4, one past the last thread) belongs to thread 3.  Fewer rows than threads: one block."""
    f = lambda r, n, b, t: int(R.first_row(r, n, b, t))
    assert [f(r, 1101, 4, 4) for r in (0, 3, 4, 274, 275, 278, 279, 1099, 1100)] == [0, 0, 4, 272, 275, 275, 279, 1097, 1097]
    assert [f(r, 1101, 3, 5) for r in (219, 220, 1100)] == [219 - 219 % 3, 220, 880 + (1100 - 880) // 3 * 3]
    assert [f(r, 3, 4, 4) for r in (0, 1, 2)] == [0, 0, 0]
    assert [f(r, 3, 2, 4) for r in (0, 1, 2)] == [0, 0, 2]


@pytest.mark.parametrize("P", R.AH_WIDTHS)
def test_csr_stage_equals_oracle(oracle, P):
    """The A.H stage on the graph with its hostile rows.  The oracle runs whole layers: its X is the sparse identity, so its
    H is the table (one product by 1 per element, -0 stored as +0, which no sum can tell apart)."""
    g, _ = R.hostile_graph()
    T = R.table(P)
    eye = _eye_csr(R.N_COLS)
    for sb in R.AH_BLOCKS:
        for relu in (0, 1):
            D, Hm = oracle.layer_refhalf(0, relu, g, eye, np.ascontiguousarray(T.T), N=len(g[0]) - 1, M_adj=R.N_COLS,
                                         spmm_block=sb, return_h=True)
            want, want_h = R.layer(g, eye, np.ascontiguousarray(T.T), relu, sb)
            assert _same(want_h, Hm) and np.array_equal(want_h, T)
            assert _same(want, D)
            assert _same(want, R.csr_stage(*g, T, sb, 1, relu))


@pytest.mark.parametrize("n,M,P", R.DENSE_CASES)
def test_dense_stage_equals_oracle(oracle, n, M, P):
    x, wt = R.dense_case(n, M, P)
    eye = _eye_csr(n)
    for sb in R.DENSE_BLOCKS:
        D, Hm = oracle.layer_refhalf(1, 0, eye, x, wt, spmm_block=sb, return_h=True)
        want = R.dense_stage(x, wt, sb)
        assert _same(want, Hm)
        assert _same(R.csr_stage(*eye, want, sb), D)
    assert np.isposinf(want[R.DENSE_INF_ROW]).all() and np.isnan(want[R.DENSE_NAN_ROW]).all()
    assert np.isfinite(np.delete(want, [R.DENSE_INF_ROW, R.DENSE_NAN_ROW], axis=0)).all()


@pytest.mark.parametrize("n,M,P,sparse,sb,ft,at", R.LAYER_CASES)
def test_layer_with_thread_splits_equals_oracle(oracle, n, M, P, sparse, sb, ft, at):
    adj, fea, wt = R.layer_case(n, M, P, sparse)
    for relu in (0, 1):
        D, Hm = oracle.layer_refhalf(0 if sparse else 1, relu, adj, fea, wt, spmm_block=sb, fea_threads=ft, adj_threads=at,
                                     return_h=True)
        want, want_h = R.layer(adj, fea, wt, relu, sb, ft, at)
        assert _same(want_h, Hm)
        assert _same(want, D)


def _moved(mutant, want):
    return float((R.bits(mutant) != R.bits(want)).mean())


def test_each_piece_of_the_arithmetic_is_observable():
    """adj_graph() at spmm_block 4, 40 columns: replacing one piece of the restatement changes more than 1 % of the outputs,
    so a kernel that got that piece wrong cannot pass.  The unclamped remainder is shown with 100 threads (blocks of 5 rows,
    98 rows left to the last thread, which an unclamped index cuts into blocks of 5 again)."""
    g = R.adj_graph()
    T = R.table(40)
    want = R.csr_stage(*g, T, 4)
    f64 = np.float64
    mutants = {
        "phase 0 for every row": dict(_first_row=lambda r, n, b, t: r),
        "fold (p0+p1)+(p2+p3)": dict(_fold=lambda p: (p[0] + p[1]) + (p[2] + p[3])),
        "product and add in one rounding": dict(_mac=lambda p, v, t: (p.astype(f64) + v.astype(f64) * t.astype(f64)).astype(R.H)),
    }
    for name, hook in mutants.items():
        assert _moved(R.csr_stage(*g, T, 4, **hook), want) > 0.01, name

    def unclamped(r, n, b, t):
        first = r // (n // t) * (n // t)
        return first + (r - first) // b * b
    want = R.csr_stage(*g, T, 4, threads=100)
    assert _moved(R.csr_stage(*g, T, 4, threads=100, _first_row=unclamped), want) > 0.01
    # and the dense stream: phase and clamp (the arithmetic is the same mac and fold)
    x, wt = R.dense_case(1199, 41, 24)                                 # 100 threads: blocks of 11, 110 rows to the last
    want = R.dense_stage(x, wt, 3, 100)
    assert _moved(R.dense_stage(x, wt, 3, 100, _first_row=lambda r, n, b, t: r), want) > 0.01
    assert _moved(R.dense_stage(x, wt, 3, 100, _first_row=unclamped), want) > 0.01


def test_hostile_rows_hold_what_they_say():
    g, rows = R.hostile_graph()
    rp, ci, va = g
    T = R.table(24)
    assert np.isfinite(va.astype(np.float32)).all() and np.isfinite(T.astype(np.float32)).all()      # overflow arises in the sums
    with np.errstate(over="ignore"):
        prods = va[:, None].astype(R.H) * T[ci]
    assert np.isfinite(prods.astype(np.float32)).all()
    for sb in R.AH_BLOCKS:
        raw, act = R.csr_stage(*g, T, sb), R.csr_stage(*g, T, sb, relu=True)
        assert np.isposinf(raw[rows["inf"]]).all() and np.isposinf(act[rows["inf"]]).all()
        assert np.isnan(raw[rows["nan"]]).all() and (R.bits(act[rows["nan"]]) == 0).all()
        e = slice(rp[rows["negzero"]], rp[rows["negzero"] + 1])
        assert (R.bits(prods[e]) == 0x8000).all()                         # every product is -0 ...
        assert (R.bits(raw[rows["negzero"]]) == 0).all() and (R.bits(act[rows["negzero"]]) == 0).all()   # ... the sum +0
        assert (R.bits(raw[rows["subnormal"]]) == 6).all() and (R.bits(act[rows["subnormal"]]) == 6).all()
        assert (R.bits(raw[rows["negsub"]]) == 0x8050).all() and (R.bits(act[rows["negsub"]]) == 0).all()
        others = np.delete(raw, [rows["inf"], rows["nan"]], axis=0)
        assert np.isfinite(others.astype(np.float32)).all()
    # negative values and zeros of either sign feed the ordinary rows too
    assert (R.bits(T) == 0x8000).mean() > 0.03 and (raw[:R.N_GRAPH] < 0).mean() > 0.2


def test_every_phase_occurs():
    g, _ = R.hostile_graph()
    rp = g[0].astype(np.int64)
    n = len(rp) - 1
    for sb in (2, 3, 4):
        phase = (rp[:-1] - rp[R.first_row(np.arange(n), n, sb, 1)]) % 4
        share = np.bincount(phase, minlength=4) / n
        assert share.min() >= 0.05, (sb, share)
    deg = np.diff(rp)
    assert set(range(6)) | {31, 32, 33, 63, 64, 65, 300} <= set(deg.tolist())
    assert deg[21] == 0 and deg[22] == 0 and n % 4 and R.N_GRAPH % 4
