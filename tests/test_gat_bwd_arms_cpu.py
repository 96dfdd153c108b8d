"""The graphs of tests/_gat_bwd_graphs.py and what tests/test_gpu_gat_bwd_arms.py rests on, without a GPU: the builder's
invariants, that the width lists reach every lane-group arm of the three backward kernels, that the statistics half's
"left out" cap holds for the float64 restatement alone, and that four plausible kernel errors, restated in numpy on the
same inputs, fall outside _gat_ref.backward_edges' bounds on a named row."""
import numpy as np
import pytest

import _gat_bwd_graphs as B
import _gat_ref as R

ALL_LANES = {1, 2, 4, 8, 16, 32, 64}


@pytest.fixture(scope="module")
def main():
    return B.adversarial("f32")


def _row(g, name):
    return next(r for r, n in g["names"].items() if n == name)


def _check_csr(g):
    rp = g["rowptr"]
    assert rp[0] == 0 and (np.diff(rp) >= 0).all() and rp[-1] == g["nnz"] == len(g["col"]) == len(g["val"])
    assert len(rp) == g["n_rows"] + 1 and g["n_cols"] >= g["n_rows"]
    assert (g["col"] >= 0).all() and (g["col"] < g["n_cols"]).all() and np.isfinite(g["val"]).all()
    tail = g["capacity"] - g["nnz"]
    assert tail > 0 and len(g["col_cap"]) == len(g["val_cap"]) == g["capacity"]
    assert np.array_equal(g["col_cap"][:g["nnz"]], g["col"]) and np.array_equal(g["val_cap"][:g["nnz"]], g["val"], equal_nan=True)
    assert (g["col_cap"][g["nnz"]:] >= g["n_cols"]).all() and np.isnan(g["val_cap"][g["nnz"]:]).all()
    assert len(g["score_row"]) == g["n_rows"] and len(g["score_col"]) == g["n_cols"]


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_main_graph_has_the_named_rows_where_stated(dt):
    g = B.adversarial(dt)
    _check_csr(g)
    deg = np.diff(g["rowptr"])
    n = g["n_rows"]
    for k in B.ROW_LENGTHS:
        assert deg[_row(g, f"len{k}")] == k
    for edge in (B.ROW_LANES, B.WINDOW, B.LONG_ROW_CUT, B.LONG_THREADS):
        assert {edge - 1, edge, edge + 1} <= set(B.ROW_LENGTHS)
    assert 2 * B.LONG_THREADS + 1 in B.ROW_LENGTHS                 # a third trip of the long row's 1024 threads
    # empty rows first and in runs; the long rows of ROW_LENGTHS share the first window
    assert (deg[:3] == 0).all() and (deg[_row(g, "empty_run_0"):_row(g, "empty_run_4") + 1] == 0).all()
    assert sum(deg[:B.WINDOW] > B.LONG_ROW_CUT) >= 2
    # a long row as the very last row and another one in the same, ragged, last window
    last_window = (n - 1) // B.WINDOW * B.WINDOW
    assert n % B.WINDOW != 0 and _row(g, "long_last_row") == n - 1 and deg[n - 1] > B.LONG_ROW_CUT
    assert _row(g, "long_in_last_window") >= last_window and deg[_row(g, "long_in_last_window")] > B.LONG_ROW_CUT
    assert g["nnz"] % 64 != 0 and g["nnz"] % 256 != 0
    # masks
    live = g["val"] > 0
    sl = lambda name: slice(g["rowptr"][_row(g, name)], g["rowptr"][_row(g, name) + 1])
    v = g["val"][sl("mask_edge_values")]
    assert v[1] == 0 and not np.signbit(v[1]) and v[2] == 0 and np.signbit(v[2]) and (v[3] < 0 or dt == "f16" and v[3] <= 0)
    assert 0 > v[3] > -2.0 ** -14 if dt == "f16" else 0 > v[3] > -2.0 ** -126
    assert not live[sl("dead_short")].any() and not live[sl("dead_long")].any() and deg[_row(g, "dead_long")] > B.LONG_ROW_CUT
    # E exactly +0.0 and -0.0 on live entries, in a short row and in one over the cut
    ref = B.forward_ref(g)
    E32 = ref["E"].astype(np.float32)
    plus, minus = g["zero_cols"]
    for name in ("zero_scores", "zero_scores_long"):
        s = sl(name)
        zp, zm = g["col"][s] == plus, g["col"][s] == minus
        assert zp.sum() >= 2 and zm.sum() >= 2 and live[s][zp | zm].all()
        assert (E32[s][zp] == 0).all() and not np.signbit(E32[s][zp]).any()
        assert (E32[s][zm] == 0).all() and np.signbit(E32[s][zm]).all()
        assert (ref["S"][s][zp | zm] > 1e-4).all()
    assert deg[_row(g, "zero_scores_long")] > B.LONG_ROW_CUT >= deg[_row(g, "zero_scores")]
    # the special columns are stored nowhere else
    special = np.isin(g["col"], [plus, minus])
    assert set(ref["row"][special]) == set(g["zero_rows"])


def test_small_variants():
    t = B.tiny("f32")
    _check_csr(t)
    assert 0 < t["nnz"] < 64 and np.diff(t["rowptr"])[0] == 0 and np.diff(t["rowptr"])[-1] == 0
    z = B.no_entries("f16")
    _check_csr(z)
    assert z["n_rows"] > 0 and z["nnz"] == 0
    m = B.many_entries(256)
    _check_csr(m)
    assert m["nnz"] > B.DOT_BLOCK * B.DOT_BLOCKS_PER_CU * 256 and (np.diff(m["rowptr"]) == 9).all()


def test_many_rows_places_its_long_rows_in_the_stated_windows():
    g = B.many_rows()
    _check_csr(g)
    n = g["n_rows"]
    assert n == g["n_cols"] == 70_001
    rps = B.rows_per_slice(n)
    assert rps == -(-n // min(1024, -(-n // 64))) == 69 and rps > B.WINDOW          # a run is more than one window
    deg = np.diff(g["rowptr"])
    where = {}
    for name, (r, k) in g["placed"].items():
        assert deg[r] == k > B.LONG_ROW_CUT and g["names"][r] == name
        run, at = divmod(r, rps)
        n_windows = -(-(min((run + 1) * rps, n) - run * rps) // B.WINDOW)
        where[name] = (run, at // B.WINDOW, at % B.WINDOW, n_windows)
    assert where["run3_first_row"] == (3, 0, 0, 2)
    assert where["run3_first_window_last_row"] == (3, 0, 63, 2)
    assert where["run3_last_window_first_row"] == (3, 1, 0, 2)
    assert where["run500_last_row"] == (500, 1, rps - 65, 2)
    assert where["last_row"][0] == (n - 1) // rps and g["placed"]["last_row"][0] == n - 1
    others = np.ones(n, bool)
    others[[r for r, _k in g["placed"].values()]] = False
    assert deg[others].max() <= 3 and deg[others].min() == 0
    h = B.hub(70_001)
    _check_csr(h)
    dh = np.diff(h["rowptr"])
    for F, pair in ((64, (4096, 4097)), (257, (1024, 1025))):
        assert tuple(B.attention_workers(F) * B.LONG_ROW_CUT + i for i in (0, 1)) == pair
    assert {4096, 4097, 65537} <= set(dh) and {1024, 1025} <= set(B.ROW_LENGTHS)
    assert -(-65537 // B.LONG_ROW_CUT) > B.attention_workers(4) == 256              # a second round with LPR 1


def test_width_lists_reach_every_arm():
    assert {B.edge_lanes(F) for F in B.EDGE_WIDTHS} == ALL_LANES
    assert {B.attention_lanes(F) for F in B.ATTENTION_WIDTHS} == ALL_LANES
    assert B.EDGE_WIDTHS == [1, 7, 16, 17, 32, 33, 64, 100, 129, 257, 513, 1030]
    assert B.ATTENTION_WIDTHS == [1, 4, 5, 8, 9, 20, 33, 64, 65, 129, 257, 300, 513]
    for widths, lanes in ((B.EDGE_WIDTHS, B.edge_lanes), (B.ATTENTION_WIDTHS, B.attention_lanes)):
        assert any(F % 4 for F in widths), "a ragged last 4-column group"
        assert any(F > 4 * lanes(F) for F in widths), "more than one TILE pass"
    assert max(-(-F // (4 * B.edge_lanes(F))) for F in B.EDGE_WIDTHS) > 4             # LPR 64 past four passes
    # the lane rules at their steps
    assert [B.edge_lanes(F) for F in (16, 17, 32, 33, 512, 513, 5000)] == [1, 2, 2, 4, 32, 64, 64]
    assert [B.attention_lanes(F) for F in (4, 5, 8, 9, 128, 129, 5000)] == [1, 2, 2, 4, 32, 64, 64]
    # G's alignment arm: a contiguous G of odd width, or one whose pitch is no multiple of 4, takes element loads
    assert any(F % 4 for F in B.EDGE_WIDTHS) and any(F % 4 == 0 for F in B.EDGE_WIDTHS)
    import _attention_grad_flat_ref as FR
    from test_gpu_attention_grad_flat import WIDTHS
    assert {FR.lanes(F) for F in WIDTHS} == ALL_LANES
    assert all(FR.lanes(F) == B.attention_lanes(F) for F in range(1, 600))


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_statistics_cap_holds_for_the_reference_alone(dt):
    """test_gpu_gat_stats.check_backward_from_statistics leaves out the live entries with |E| <= bE, at most 0.5 %: on
    the graph without the deliberate zero scores the restatement leaves out none."""
    g = B.adversarial(dt, zero_scores=False)
    assert g["zero_cols"] is None and g["zero_rows"] == []
    ref = B.forward_ref(g, "mean")
    unsure = ref["live"] & (np.abs(ref["E"]) <= ref["bE"])
    assert unsure.sum() == 0 <= 0.005 * ref["live"].sum()
    assert np.abs(ref["E"]).min() >= 0.2 / 8 - 1e-12
    # the scores are exact in fp32, so the statistics hold what the restatement used
    for k in ("score_row", "score_col"):
        assert np.array_equal(g[k].astype(np.float32).astype(np.float64), g[k])
    m, l = B.row_statistics(g, ref)
    assert ((l > 0) == ~ref["dead"]).all() and (m[ref["dead"]] == 0).all()
    w = np.where(ref["live"], np.exp(ref["E"] - m[ref["row"]]) / np.where(l > 0, l, 1.0)[ref["row"]], 0.0)
    live_rows = ~ref["dead"][ref["row"]]
    assert np.allclose(w[live_rows], ref["S"][live_rows], rtol=1e-12, atol=0)


# ---- mutants -----------------------------------------------------------------------------------------------------------

def edge_pass(g, E, S, G, Wh, alpha=0.2, mutant=None):
    """sgx_gat_backward_edges in float64, optionally with one kernel error:
    "rowsum_first_256"    the row sum of dx over the first 256 entries of a long row only;
    "second_long_skipped" only the first long row of a 64-row window is taken: the others keep dx in sg, g1 = 0;
    "slope_ge"            the LeakyReLU slope picked with E >= 0 instead of E > 0;
    "last_group_dropped"  the dot product without the last 4-column group of a ragged width."""
    rowptr, col, val = g["rowptr"], g["col"], g["val"]
    row, deg = R.rows_of(rowptr), np.diff(rowptr)
    F = Wh.shape[1]
    cut = (F - 1) // 4 * 4 if mutant == "last_group_dropped" else F
    d = np.einsum("ek,ek->e", G[row][:, :cut], Wh[col][:, :cut])
    dx = S * d
    if mutant == "rowsum_first_256":
        k = np.arange(len(col)) - rowptr[row]
        rs = R._seg(np.add, np.where((deg[row] <= B.LONG_ROW_CUT) | (k < 256), dx, 0.0), rowptr, 0.0)
    else:
        rs = R._seg(np.add, dx, rowptr, 0.0)
    slope = np.where(E >= 0 if mutant == "slope_ge" else E > 0, 1.0, float(np.float32(alpha)))
    sg = np.where(val > 0, (dx - S * rs[row]) * slope, 0.0)
    g1 = R._seg(np.add, sg, rowptr, 0.0)
    if mutant == "second_long_skipped":
        for w0 in range(0, len(deg), B.WINDOW):
            for r in (w0 + np.nonzero(deg[w0:w0 + B.WINDOW] > B.LONG_ROW_CUT)[0])[1:]:
                sg[rowptr[r]:rowptr[r + 1]] = dx[rowptr[r]:rowptr[r + 1]]
                g1[r] = 0.0
    return sg, g1


@pytest.fixture(scope="module")
def edge_case(main):
    F = 7
    ref = B.forward_ref(main)
    E, S = (ref[k].astype(np.float32).astype(np.float64) for k in ("E", "S"))
    Wh, G = B.edge_tables(main, F)
    return E, S, G, Wh, R.backward_edges(main, E, S, G, Wh)


def _named_rows_outside(g, got, want, bound, row_of):
    bad = ~(np.abs(got - want) <= bound)
    return {g["names"][r] for r in set(row_of[bad].tolist()) if r in g["names"]}


def test_the_restatement_without_a_mutation_is_inside_the_bounds(main, edge_case):
    E, S, G, Wh, (want_sg, want_g1, b_sg, b_g1) = edge_case
    sg, g1 = edge_pass(main, E, S, G, Wh)
    R.check("sg", sg, want_sg, b_sg, R.rows_of(main["rowptr"]), main["names"])
    R.check("g1", g1, want_g1, b_g1, np.arange(main["n_rows"]), main["names"])


@pytest.mark.parametrize("mutant,rows", [
    ("rowsum_first_256", {"len257", "len1023", "len2049", "long_last_row", "zero_scores_long"}),
    ("second_long_skipped", {"len1023", "len2049", "long_last_row"}),
    ("slope_ge", {"zero_scores", "zero_scores_long"}),
    ("last_group_dropped", {"len7", "len9", "len257", "long_last_row"}),      # (a row of one entry has sg = 0 whatever d is)
])
def test_mutants_fall_outside_the_bounds_on_named_rows(main, edge_case, mutant, rows):
    E, S, G, Wh, (want_sg, want_g1, b_sg, b_g1) = edge_case
    sg, g1 = edge_pass(main, E, S, G, Wh, mutant=mutant)
    hit = _named_rows_outside(main, sg, want_sg, b_sg, R.rows_of(main["rowptr"]))
    hit |= _named_rows_outside(main, g1, want_g1, b_g1, np.arange(main["n_rows"]))
    print(mutant, "outside the bounds on", sorted(hit))
    assert rows <= hit, (mutant, sorted(rows - hit))
    if mutant == "slope_ge":
        assert hit == rows                               # nothing but the zero scores tells > from >=
    if mutant == "second_long_skipped":
        assert "len257" not in hit                       # the first long row of its window is taken


def test_a_long_row_left_out_of_many_rows_is_outside_both_attention_bounds():
    """What a stale mask word or a skipped window would do to the attention gradient: each placed long row of "many_rows"
    left out of the float64 sum moves the entries' half past the row form's bound and the entry-split form's."""
    import _attention_grad_flat_ref as FR
    g = B.many_rows()
    F = 20
    sg, g1 = B.attention_inputs(g["rowptr"], g["col_cap"], g["nnz"], seed=9)
    assert np.isnan(sg[g["nnz"]:]).all() and np.isfinite(sg[:g["nnz"]]).all()
    Wh = np.random.default_rng(1).uniform(-1, 1, (g["n_cols"], F)).astype(np.float32)
    want, mag = FR.exact(g["rowptr"], g["col"], sg, g1, Wh)
    rows = B.attention_bound(F, g["rowptr"], mag)
    flat = np.maximum(FR.bound(g["rowptr"], 256, F, mag), FR.bound(g["rowptr"], 1024, F, mag))     # (the library's T is 256)
    for name, (r, _k) in g["placed"].items():
        cut = sg.copy()
        cut[g["rowptr"][r]:g["rowptr"][r + 1]] = 0
        err = np.abs(FR.exact(g["rowptr"], g["col"], cut, g1, Wh)[0] - want)
        assert (err[F:] > 4 * rows[F:]).any() and (err[F:] > 4 * flat[F:]).any(), name


def test_attention_bound_counts_the_chains():
    """attention_depth on shapes whose chains can be counted by hand"""
    rp = np.arange(0, 65 * 3, 3)                                       # 64 rows of 3 entries: one slice, one run of 64
    assert B.attention_depth(4, rp) == (1 + 256 + 1, 3 + 1 + 256 + 0 + 1)          # LPR 1: 256 workers, a row each
    assert B.attention_depth(257, rp) == (16 + 4 + 1, 3 + 16 + 4 + 0 + 1)          # LPR 64: 4 workers, 16 rows each
    g = B.hub(300)
    d_rows, d_ent = B.attention_depth(4, g["rowptr"])
    assert d_ent == 256 + 257 + 3 + B.attention_slices(g["n_rows"])                # 257 chunks, three long rows in the run
    assert 3 * 2.0 ** -24 > 1e-7             # the derived factor is never below test_gpu_layer_grad's TOL["grad_attention"]
