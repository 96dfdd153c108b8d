"""The net under tests/test_gpu_xw_sparse_arms.py, checked without a GPU (tests/_xw_sparse_ref.py): the restated arm selection
reaches every arm the GPU cases name, the fixtures have the properties the kernel's branches need, and the float64
reference with its derived bound has no slack where it matters -- every mutation the kernel could suffer (an entry lost, a
neighbour's entry gained through a missing select, rows or slices landing in the wrong place, a unit skipped) puts EVERY
row it touches outside the bound in at least one column.

A GPU result is within `bound` of float64, so a mutation that moves a row by more than 2 x bound in some column cannot hide
behind the kernel's own rounding: that, not 1 x bound, is what is asserted.  Rows a mutation leaves as they are (two empty
rows swapped, a slice of an empty row shifted) are not mutated rows."""
import numpy as np
import pytest

import _spmm_acc_ref as R
import _xw_sparse_ref as X

P_MUT = 64


def _arm_of(name, dt, P, **kw):
    rp = X.structure(name)[0]
    deg = np.diff(rp)
    return X.arm(dt, len(deg), X.n_cols(name), P, int(rp[-1]), int(deg.max()), **kw)


def test_case_tables_name_the_arms_the_restatement_selects():
    seen = set()
    for dt, P, cap, lpr, n_split, full in X.DEEP_CASES:
        a = _arm_of("deep", dt, P, ldw=P, lpr_cap=cap or 0)
        assert a is not None and (a.lpr, a.n_split, a.full) == (lpr, n_split, full), (dt, P, cap, a)
        assert a.streams == 8 and a.wgs_per_cu == (1 if lpr == 16 else 2)
        if cap is not None:                                  # a narrowing: the natural split is wider
            assert X.choose_lpr(dt, X.DEEP_M, P) > cap == lpr
        seen.add((dt, lpr, full, n_split))
    assert {(dt, lpr, full) for dt, lpr, full, _ in seen} == {(dt, lpr, full) for dt in ("f16", "f32") for lpr in (2, 4, 8, 16)
                                                              for full in (True, False)}
    assert {s for _, _, _, s in seen} == {1, 2, 3, 4}
    for dt in ("f16", "f32"):                               # the last slice full and ragged at more than one slice
        assert {full for d, _, full, s in seen if d == dt and s > 1} == {True, False}
    for dt, P, lpr, n_split, full in X.WIDE_CASES:
        for cap, streams in ((8, 8), (16, 16), (0, 32)):
            a = _arm_of("wide", dt, P, ldw=P, streams_cap=cap)
            assert (a.lpr, a.n_split, a.full, a.streams) == (lpr, n_split, full, streams), (dt, P, cap, a)
    assert {(dt, lpr) for dt, _, lpr, _, _ in X.WIDE_CASES} == {("f16", 2), ("f16", 8), ("f32", 4), ("f32", 16)}
    for dt, P, lpr in X.HOSTILE_CASES:
        assert _arm_of("hostile", dt, P).lpr == lpr
    assert {(dt, X.eps(lpr)) for dt, _, lpr in X.HOSTILE_CASES} == {(dt, e) for dt in ("f16", "f32") for e in (2, 4)}
    # outside the gate: under 2^20 entries, under 4096 rows, a row over the plan's cut, more than four slices, one lane
    assert X.arm("f16", 5000, 600, 64, (1 << 20) - 1, 100) is None and X.arm("f16", 4095, 600, 64, 1 << 20, 100) is None
    assert X.arm("f16", 5000, 600, 64, 1 << 20, 513) is None and X.arm("f16", 5000, 3703, 80, 1 << 20, 100) is None
    assert X.arm("f16", 5000, 700, 8, 1 << 20, 100) is None and X.arm("f32", 5000, 700, 4, 1 << 20, 100) is None


def test_window_walk_counts():
    """at 8 streams every wavefront of `wide` walks 3 windows and the first five walk 4; at 16 one or two; unset at most one"""
    assert (X.WIDE_ROWS + 63) // 64 == 389
    assert X.windows_per_wavefront(X.WIDE_ROWS, 8) == [4] * 5 + [3] * 123
    assert X.windows_per_wavefront(X.WIDE_ROWS, 16) == [2] * 133 + [1] * 123
    assert max(X.windows_per_wavefront(X.WIDE_ROWS, 32)) == 1
    assert max(X.windows_per_wavefront(X.DEEP_ROWS, 8)) == 1


def test_fixture_deep():
    rp, ci, va = X.matrix("deep", "f16")
    deg = np.diff(rp)
    n, nnz = len(deg), int(rp[-1])
    assert 4096 <= n < 4800 and n % 64 == 37 and nnz >= 1 << 20 and nnz % 2 == 1 and nnz < 1 << 22
    assert deg.max() == X.PLAN_CUT and deg[-2] == 0 and deg[-1] > 0
    for w, want in enumerate(X.DEEP_WINDOWS):
        assert deg[64 * w:64 * w + 64].tolist() == want
    assert (deg[:64] == 0).all() and deg[64:128].tolist() == [0] * 63 + [512] and (deg[128:192] == 32).all()
    assert deg[192:256].tolist() == list(range(64))
    edge = deg[256:320].tolist()
    for u in (16, 32):                                       # both unit sizes: one, two, three units, one less, one more
        for d in (u - 1, u, u + 1, 2 * u - 1, 2 * u, 2 * u + 1, 3 * u, 3 * u + 1):
            assert d in edge
    assert all(d in edge for d in (1, 2, 3, 4, 5, 7, 8, 9)) and edge.count(0) == 64 - 24
    fill = deg[64 * len(X.DEEP_WINDOWS):-2]
    assert fill.min() >= 250 and fill.max() <= 270
    # an all-empty last sub-tile behind sub-tiles with steps, for every lane split; exactly one such sub-tile at LPR 16, 4, 2
    orders = X.win_order(deg)
    for lpr in (2, 4, 8, 16):
        rpw = 64 // lpr
        ranked = [deg[64 * w + orders[w]] for w in range(len(X.DEEP_WINDOWS))]
        assert any(d[64 - rpw] == 0 and d[0] > 0 for d in ranked), lpr
        assert lpr == 8 or any(d[64 - rpw] == 0 and d[64 - rpw - 1] > 0 for d in ranked), lpr
    _check_entries(rp, ci, va, X.DEEP_M)


def test_fixture_wide():
    rp, ci, va = X.matrix("wide", "f32")
    deg = np.diff(rp)
    assert len(deg) == 64 * (3 * 128 + 5) - 27 and rp[-1] >= 1 << 20 and deg.max() <= 200 < X.PLAN_CUT
    longs = deg[::97]
    assert longs.min() >= 129 and longs.max() <= 200
    rest = np.delete(deg, np.arange(0, len(deg), 97))
    assert set(np.unique(rest)) <= {0, *range(20, 71)} and 0.03 < (rest == 0).mean() < 0.07
    _check_entries(rp, ci, va, X.WIDE_M)


def _check_entries(rp, ci, va, M):
    assert ci.min() >= 0 and ci.max() < M
    inside = np.ones(len(ci), bool)
    inside[rp[1:-1][rp[1:-1] < len(ci)]] = False             # first entries of rows
    inside[0] = False
    assert (np.diff(ci.astype(np.int64))[inside[1:]] > 0).all()       # distinct and sorted inside a row
    fin = np.isfinite(va)
    assert (np.abs(va[fin]) >= 0.25).all() and (np.abs(va[fin]) <= 1.0).all()


def test_fixture_hostile():
    rp, ci, va = X.matrix("hostile", "f16")
    deg = np.diff(rp)
    chosen, before = X.hostile_rows()
    assert rp[-1] >= 1 << 20 and deg.max() == X.PLAN_CUT and len(deg) == X.DEEP_ROWS
    assert len({r // 64 for r in chosen}) == len(chosen) == 6 and any(r % 64 == 0 for r in chosen)
    assert sorted(deg[before].tolist()) == [1, 1, 3, 3, 5, 5] and deg[chosen].max() <= 13 and deg[chosen].min() >= 6
    assert deg[-2] == 1 and deg[-1] > 0
    bad_val = np.nonzero(~np.isfinite(va))[0]
    assert sorted(bad_val.tolist()) == sorted(int(rp[r]) for r in X.HOSTILE_VALUE_ROWS)       # the first entry of each
    bad_col = np.nonzero(ci < len(X.HOSTILE_W))[0]
    assert sorted(bad_col.tolist()) == sorted(int(rp[r]) for r in X.HOSTILE_COLUMN_ROWS)
    # every other row of deep keeps its length
    other = np.ones(len(deg), bool)
    other[chosen + before + [len(deg) - 2, len(deg) - 1]] = False
    assert np.array_equal(deg[other], X.deep_degrees()[other])
    _check_entries(rp, ci, va, X.DEEP_M)
    for dt, P, _ in X.HOSTILE_CASES:
        want, bound, _ = X.reference("hostile", dt, P)
        rows = np.nonzero(~np.isfinite(want).all(1))[0]
        assert rows.tolist() == chosen                       # non-finite in exactly the chosen rows
        assert np.isnan(want[64 * 31 + 40]).all() and np.isnan(want[64 * 27]).all()                    # a NaN value; W[1] = NaN
        for r in (64 * 12 + 1, 64 * 20, 64 * 15 + 63, 64 * 44 + 17):                                   # +-inf by the other factor's sign
            assert np.isinf(want[r]).all() and (want[r] > 0).any() and (want[r] < 0).any()
        assert np.isfinite(bound).all()


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("name", ["deep", "wide"])
def test_mutations_land_outside_the_bound(name, dt):
    rp, ci, va = X.matrix(name, dt)
    W = X.weights(name, P_MUT, dt)
    want, bound, n = X.reference(name, dt, P_MUT)
    deg = np.diff(rp).astype(np.int64)
    nnz, n_rows = int(rp[-1]), len(deg)
    rp64 = rp.astype(np.int64)

    def caught(what, rows, mutated):
        """every row of `rows` is outside 2 x bound in at least one column"""
        rows = np.asarray(rows)
        assert len(rows) > 0, what
        out = (np.abs(mutated - want[rows]) > 2.0 * bound[rows]).any(1)
        assert out.all(), f"{name} {dt}: {what}: {int((~out).sum())} of {len(rows)} mutated rows stay inside the bound, first row {rows[~out][0]}"

    # a row's last entry dropped
    rows = np.nonzero(deg > 0)[0]
    last = rp64[rows + 1] - 1
    caught("last entry dropped", rows, want[rows] - va[last, None] * W[ci[last]])
    # the entry behind a row's end added: the next row's first entry (an over-read slot without either select)
    rows = np.nonzero(rp64[1:] < nnz)[0]
    nxt = rp64[rows + 1]
    caught("the next row's first entry added", rows, want[rows] + va[nxt, None] * W[ci[nxt]])
    # ... with the column select only missing its value: W[0] times the next entry's value
    caught("W[0] x the next entry's value added", rows, want[rows] + va[nxt, None] * W[0])
    # two rows of one window swapped (pairs 2 k, 2 k + 1; a pair of empty rows is no mutation)
    a = np.arange(0, n_rows - 1, 2)
    a = a[(deg[a] > 0) | (deg[a + 1] > 0)]
    caught("rows swapped", np.concatenate([a, a + 1]), np.concatenate([want[a + 1], want[a]]))
    # a slice's columns taken from the next slice (slices of 16 columns: fp16 LPR 2, fp32 LPR 4; of 32)
    rows = np.nonzero(deg > 0)[0]
    for cp in (16, 32):
        for s in range(P_MUT // cp - 1):
            m = want[rows].copy()
            m[:, s * cp:(s + 1) * cp] = want[rows, (s + 1) * cp:(s + 2) * cp]
            caught(f"slice {s} of {cp} columns shifted", rows, m)
    # a row's second unit skipped (units of 16 and of 32 entries)
    pos = np.arange(nnz) - np.repeat(rp64[:-1], deg)
    for u in (16, 32):
        rows = np.nonzero(deg > u)[0]
        skipped = R.subset((rp, ci, va), (pos >= u) & (pos < 2 * u))
        caught(f"second unit of {u} entries skipped", rows, want[rows] - (R.dense(skipped, len(W)) @ W)[rows])


def test_form_query_without_a_plan_is_the_gather_kernel():
    """sgx_xw_sparse_form is a host query: no plan (or a shape the launch would reject) answers 0 without a device"""
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    assert _lib.lib.sgx_xw_sparse_form(0, 5000, 600, 64, None, 64, None, 64, None) == 0
    assert _lib.lib.sgx_xw_sparse_form(7, 5000, 600, 64, None, 64, None, 64, None) == 0
    assert _lib.lib.sgx_xw_sparse_form(1, 5000, 600, 64, None, 32, None, 64, None) == 0
