"""The graph of tests/test_gpu_long_rows.py has the rows that test is about, and its float64 restatement can tell the
slope of nearly every live entry: checked with numpy alone."""
import numpy as np
import pytest

import _gat_ref as R
import _long_rows_graph as L
from test_gpu_gat_stats import MAX_LEFT_OUT


@pytest.mark.parametrize("heads,f_head", [(1, 16), (8, 4)])
@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_the_graph_has_the_rows_the_walk_is_tested_on(dt, heads, f_head):
    g = L.graph(dt, heads, f_head)
    deg = np.diff(g["rowptr"])
    n = g["n_rows"]
    assert n == len(deg) == 150 and n % 8 != 0 and n % 64 != 0 and g["n_cols"] >= n
    is_long = deg > L.CUT
    assert (deg == 256).sum() == 1 and (deg == 257).sum() == 1 and not is_long[deg == 256].any() and is_long[deg == 257].all()
    assert is_long[0] and is_long[1] and 0 // 8 == 1 // 8                  # two long rows next to each other in one window of 8
    assert is_long[64] and 64 % 64 == 0 and 64 % 8 == 0                    # the first row of a window, at both spans
    assert is_long[n - 1] and (n - 1) // 8 == n // 8 and (n - 1) // 64 == n // 64   # the last row, in the partial window
    assert is_long[64] and deg[65] == 0 and is_long[66]                    # an empty row between long rows
    assert set(np.nonzero(is_long)[0]) == {r for r, v in L.NAMED.items() if v[1] > L.CUT}
    assert deg[~is_long].max() == 256 and np.delete(deg, list(L.NAMED)).max() <= 12
    ref = R.forward(g, heads, dead_rule="mean", out=dt)
    live_per_row = R._seg(np.add, ref["live"].astype(np.int64), g["rowptr"], 0)
    assert is_long[70] and live_per_row[70] == 0 and ref["dead"][70]       # the dead long row
    assert (live_per_row[is_long] > 0).sum() == is_long.sum() - 1 and (~ref["live"]).sum() > deg[70]
    assert np.array_equal(ref["dead"], live_per_row == 0)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_the_restatement_leaves_out_few_entries(dt):
    g = L.graph(dt, 1, 16)
    ref = R.forward(g, 1, dead_rule="mean", out=dt)
    unsure = ref["live"] & (np.abs(ref["E"]) <= ref["bE"])
    assert unsure.sum() <= MAX_LEFT_OUT * ref["live"].sum()
