"""tests/_spmm_acc_ref.py checked on the CPU: a numpy restatement of what the kernels do per output element -- an fp32 fma
chain in edge order, the second pass starting from the first pass's fp32 sums, one rounding to the storage type -- stays
inside the derived bounds against the float64 reference on the graphs and tables the GPU tests use (R.GRAPHS), and a
dropped or doubled edge of a ten-edge row does not."""
import numpy as np
import pytest

import _spmm_acc_ref as R


def _final(acc, dt, relu=True):
    acc = np.maximum(acc, 0) if relu else acc
    return acc.astype(R.NP_DTYPE[dt]).astype(np.float64)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("name,P", [("base", 1), ("base", 7), ("base", 64), ("split", 41), ("tail", 32)])
def test_fma_chain_stays_inside_the_bounds(name, dt, P):
    """on the graphs and tables of tests/test_gpu_spmm_acc_arms.py (R.GRAPHS, R.graph_table)"""
    A, A1, A2 = R.GRAPHS[name](dt)
    n_cols = R.N_COLS[name]
    H = R.graph_table(name, P, dt)
    assert np.array_equal(R.dense(A, n_cols), R.dense(A1, n_cols) + R.dense(A2, n_cols))
    assert (A1[1] < n_cols // 2).all() and (A2[1] >= n_cols // 2).all()
    d1, d2 = np.diff(A1[0]), np.diff(A2[0])
    assert ((d1 == 0) & (d2 > 0)).sum() > 100 and ((d1 > 0) & (d2 == 0)).sum() > 100 and ((d1 == 0) & (d2 == 0)).sum() > 20
    s1, scale1, n1 = R.one_pass(A1, H)
    part = R.fma_chain_f32(A1, H)
    R.assert_within("partial", part, s1, R.partial_bound(n1, scale1))
    assert not part[d1 == 0].any()
    want, bound = R.finished(*R.second_pass(part, A2, H), dt, True)
    got = _final(R.fma_chain_f32(A2, H, acc_in=part), dt)
    R.assert_within("final", got, want, bound)
    assert np.array_equal(got[d2 == 0], _final(part[d2 == 0], dt))
    # the single pass over all of A obeys the one-pass bound too
    s, scale, n = R.one_pass(A, H)
    R.assert_within("single", _final(R.fma_chain_f32(A, H), dt), *R.finished(s, R.partial_bound(n, scale), dt, True))


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_a_dropped_or_doubled_edge_is_far_outside(dt):
    rng = np.random.default_rng(9)
    A = R.random_rows(rng, np.full(50, 10), 0, 400, dt)
    H = R.table(rng, 400, 16, dt)
    s, scale, n = R.one_pass(A, H)
    bound = R.partial_bound(n, scale)
    fbound = R.finished(s, bound, dt, False)[1]
    for factor in (0.0, 2.0):                                         # edge 3 of every row dropped / counted twice
        va = A[2].copy()
        va[A[0][:-1] + 3] *= factor
        bad = R.fma_chain_f32((A[0], A[1], va), H)
        excess = np.abs(bad - s) / bound
        assert np.median(excess.max(1)) > 1e4
        assert np.median((np.abs(_final(bad, dt, False) - s) / fbound).max(1)) > (50 if dt == "f16" else 1e4)
        with pytest.raises(AssertionError):
            R.assert_within("mutant", bad, s, bound)


def test_any_order_of_the_sum_is_inside_the_bound():
    """the split path adds a long row's chunks in another order: reversed edges and pairwise halves stay inside too"""
    rng = np.random.default_rng(11)
    A = R.random_rows(rng, [1400, 513, 65], 0, 1500, "f16")
    H = R.table(rng, 1500, 8, "f16")
    s, scale, n = R.one_pass(A, H)
    rp, ci, va = A
    rev = np.concatenate([np.arange(rp[i + 1] - 1, rp[i] - 1, -1) for i in range(3)])
    R.assert_within("reversed", R.fma_chain_f32((rp, ci[rev], va[rev]), H), s, R.partial_bound(n, scale))
    chunks = np.zeros((3, 8), np.float32)
    for i in range(3):
        parts = [R.fma_chain_f32((np.array([0, min(64, rp[i + 1] - e)], np.int32), ci[e:e + 64], va[e:e + 64]), H)[0]
                 for e in range(rp[i], rp[i + 1], 64)]
        for p in parts:
            chunks[i] = (chunks[i].astype(np.float64) + p).astype(np.float32)
    R.assert_within("chunked", chunks, s, R.partial_bound(n, scale))
