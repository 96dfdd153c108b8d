"""The long-row walk the GAT training path's kernels share (csrc/long_rows.h) at its edges, on the 150-row graph of
tests/_long_rows_graph.py (tests/test_long_rows_graph_cpu.py confirms its rows): a partial last window at both spans, rows
of exactly 256 and 257 entries, two long rows in one window of 8, a long row first in a window and one as the last row of
the graph, a dead long row, an empty row between long rows.  The statistics, both forms of the edge backward and the
attention gradient against the float64 restatements and bounds of the tests that cover those kernels elsewhere."""
import numpy as np
import pytest
import torch

import _gat_ref as R
import _long_rows_graph as L
from test_gpu_gat_stats import check_backward_from_statistics
from test_gpu_layer_backward import attention_grad_check

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
DTYPES = {"f16": torch.float16, "f32": torch.float32}


def _device(g, dt):
    from sgracex1_amd import ops
    tdt = DTYPES[dt]
    A = ops.Csr(torch.as_tensor(g["rowptr"], dtype=torch.int32, device=dev), torch.as_tensor(g["col"], dtype=torch.int32, device=dev),
                torch.as_tensor(g["val"]).to(tdt).to(dev), g["n_cols"])
    return A, torch.as_tensor(g["Wh"]).to(tdt).to(dev), torch.as_tensor(g["att"]).to(tdt).to(dev)


def _forward(g, dt, heads):
    """(A, Wh, stats, E, S, ref) with the statistics checked as tests/test_gpu_gat_stats.py checks them."""
    from sgracex1_amd import ops
    A, Wh, att = _device(g, dt)
    ref = R.forward(g, heads, dead_rule="mean", out=dt)
    D, stats = ops.gat_aggregate(A, Wh, att, alpha=0.2, heads=heads, fill_dead_rows=True, want_row_stats=True)
    E, S = ops.gat_edge_outputs(A, stats, alpha=0.2, dead_weight=1.0 / g["n_cols"])
    for name, t in (("D", D), ("E", E), ("S", S), *zip(("score_row", "score_col", "row_max", "row_sum"), stats.tensors())):
        assert torch.isfinite(t).all(), f"{name}: not finite"
    R.check_forward({"D": D.double().cpu().numpy(), "E": E.double().cpu().numpy(), "S": S.double().cpu().numpy()}, ref, g["names"])
    dead = torch.as_tensor(ref["dead"], device=dev)
    assert bool(dead[70]) and torch.equal(A.dead_rows, dead)
    l0 = stats.row_sum.reshape(g["n_rows"], heads) == 0
    assert torch.equal(l0, dead[:, None].expand(-1, heads)), "row_sum == 0 is not exactly the dead rows"
    assert not stats.row_max.reshape(g["n_rows"], heads)[dead].any()
    _D2, stats2 = ops.gat_aggregate(A, Wh, att, alpha=0.2, heads=heads, fill_dead_rows=True, want_row_stats=True)
    assert all(torch.equal(a, b) for a, b in zip(stats.tensors(), stats2.tensors())), "not the same bits on a second run"
    return A, Wh, stats, E, S, ref


@pytest.mark.parametrize("dt", list(DTYPES))
def test_statistics_of_eight_heads(dt):
    """8 heads of 4 columns: one block of heads per long row, every head's state through the workgroup's merge."""
    _forward(L.graph(dt, 8, 4), dt, 8)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_statistics_edge_backward_and_attention_gradient(dt):
    from sgracex1_amd import ops
    f_head = 16
    g = L.graph(dt, 1, f_head)
    A, Wh, stats, E, S, ref = _forward(g, dt, 1)
    # from the statistics: the comparison and bound of test_gpu_gat_stats.py (same bits on a second run included)
    G, _sg, _g1, _S_out = check_backward_from_statistics(g, ref, A, stats, Wh, f_head, True, 1.0 / g["n_cols"], ("long_rows", dt))
    # from E and S: the comparison of test_gpu_gat_paths.py, the restatement fed the kernel's own fp32 E and S
    Whf, dead = Wh.float(), A.dead_rows
    sg, g1 = ops.gat_backward_edges(A, E, S, G, Whf, alpha=0.2, dead=dead)
    sg2, g12 = ops.gat_backward_edges(A, E, S, G, Whf, alpha=0.2, dead=dead)
    assert torch.equal(sg, sg2) and torch.equal(g1, g12), "not the same bits on a second run"
    want = R.backward_edges(g, E.cpu().numpy(), S.cpu().numpy(), G.cpu().numpy(), g["Wh"], dead=dead.cpu().numpy())
    R.check("sg", sg.double().cpu().numpy(), want[0], want[2], R.rows_of(g["rowptr"]), g["names"])
    R.check("g1", g1.double().cpu().numpy(), want[1], want[3], np.arange(g["n_rows"]), g["names"])
    # the attention gradient of that edge pass: the comparison of test_gpu_layer_backward.py
    attention_grad_check(A, sg, g1, Whf, ("long_rows", dt))
