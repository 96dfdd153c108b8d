"""The plan's row schedule (csrc/row_schedule.h: tasks, lane-group rows, the degree order's one-step tail 64 rows to a
wavefront) at its edges, for the three kernels that walk it -- the plain aggregation (spmm_csr.hip), the GAT aggregate's second
stage (gat_weighted.hip) and its one-walk form (gat_fused.hip): a tail of exactly 4096 rows (taken) and of 4095 (not taken), a
grid without row blocks, a grid without tasks; at a width one pass covers, one it does not, and an fp32 one.  Every output has
the bits of the same call with the tail switched off (SGX_SPMM_NO_SHORT_TAIL), the same bits twice, and lies within
tests/test_gpu_short_tail.py's tolerances of a float64 result."""
import numpy as np
import pytest
import torch

import _gat_ref as R
import _row_schedule_graphs as G

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")

SHAPES = [("f16", 64), ("f16", 100), ("f32", 32)]         # (f16, 100): more columns than one pass of the GAT kernels' lanes covers
DTYPES = {"f16": torch.float16, "f32": torch.float32}
TOL = {"f16": dict(rtol=1e-2, atol=2e-3), "f32": dict(rtol=2e-5, atol=2e-5)}
# eight heads where the width has them (100 columns: four heads of 25)
HEADS = {64: (1, 8), 100: (1, 4), 32: (1, 8)}


class Case:
    def __init__(self, case, dt):
        from sgracex1_amd import _lib, ops
        self.g = g = G.graph(case, dt)
        tdt = DTYPES[dt]
        self.A = ops.Csr(torch.as_tensor(g["rowptr"], device=dev), torch.as_tensor(g["col"], device=dev),
                         torch.as_tensor(g["val"]).to(tdt).to(dev), g["n"])
        with _lib.tuning(SGX_PLAN_REORDER_BELOW="2"):           # (so small a graph is ordered whatever its utilisation)
            plan = ops.Plan(self.A.rowptr)
        self.A._plan = self.A._gat_plan = plan
        # the plan is the one the cases are about: in degree order, its tail counted here from the degrees
        deg = g["deg"]
        n_multi, n_one = G.tail_rows(deg)
        long_rows = G.CASES[case][2]
        assert plan.reordered and plan.long_threshold == G.SMALL_CUT and plan.long_rows == len(long_rows)
        order = plan.export("row_order").cpu().numpy()
        assert len(order) == n_multi + n_one == g["n"] - len(long_rows)
        assert (deg[order[:n_multi]] > 8).all() and (deg[order[n_multi:]] <= 8).all()
        assert sorted(order.tolist()) == np.nonzero(deg <= G.SMALL_CUT)[0].tolist()
        assert (n_one >= G.TAIL_GATE) == (case != "tail_4095") and (n_multi == 0) == (case == "tail_only")
        assert (deg == 0).any() and (deg == 8).any()


@pytest.fixture(scope="module")
def cases():
    store = {}

    def get(case, dt):
        if (case, dt) not in store:
            store[(case, dt)] = Case(case, dt)
        return store[(case, dt)]
    return get


def _three_ways(fn):
    """fn() with the tail, again, and with the tail switched off: the same bits each time; returns the first"""
    from sgracex1_amd import _lib
    got, again = fn(), fn()
    with _lib.tuning(SGX_SPMM_NO_SHORT_TAIL="1"):
        off = fn()
    for a, b, c in zip(got, again, off):
        assert torch.equal(a, b), "run to run"
        assert torch.equal(a, c), "against the sblock walk of the tail"
    return got


def _close(got, want, dt):
    np.testing.assert_allclose(got.double().cpu().numpy(), want, **TOL[dt])


@pytest.mark.parametrize("dt,width", SHAPES)
@pytest.mark.parametrize("case", list(G.CASES))
def test_plain_aggregation_at_the_schedules_edges(cases, case, dt, width):
    from sgracex1_amd import ops
    c = cases(case, dt)
    g, A = c.g, c.A
    Hd = G.table(g["n"], width, seed=width)
    H = torch.as_tensor(Hd).to(DTYPES[dt]).to(dev)
    row = torch.as_tensor(R.rows_of(g["rowptr"].astype(np.int64)))
    want = torch.zeros((g["n"], width), dtype=torch.float64)
    want.index_add_(0, row, torch.as_tensor(g["val"])[:, None] * torch.as_tensor(Hd)[torch.as_tensor(g["col"]).long()])
    (D,) = _three_ways(lambda: (ops.spmm(A, H, relu=True),))
    _close(D, want.clamp(min=0).numpy(), dt)
    # two-pass aggregation: fp32 partial sums out, then in -- twice the sum
    part, fin = _three_ways(lambda: (lambda p: (p, ops.spmm_acc(A, H, relu=True, acc_in=p)))(ops.spmm_acc(A, H, partial_out=True)))
    np.testing.assert_allclose(part.double().cpu().numpy(), want.numpy(), **TOL["f32"])
    _close(fin, (2 * want).clamp(min=0).numpy(), dt)
    assert not D[torch.as_tensor(g["deg"] == 0)].any()


@pytest.mark.parametrize("dt,width", SHAPES)
@pytest.mark.parametrize("case", list(G.CASES))
def test_gat_aggregate_at_the_schedules_edges(cases, case, dt, width):
    from sgracex1_amd import _lib, ops
    c = cases(case, dt)
    g, A = c.g, c.A
    for heads in HEADS[width]:
        Whd = G.table(g["n"], width, seed=width + heads, scale=0.5)
        attd = G.table(1, 2 * width, seed=heads, scale=0.5)[0]
        Wh = torch.as_tensor(Whd).to(DTYPES[dt]).to(dev)
        att = torch.as_tensor(attd).to(DTYPES[dt]).to(dev)
        ref = R.forward(dict(rowptr=g["rowptr"], col=g["col"], val=g["val"], Wh=Whd, att=attd), heads, relu=True,
                        dead_rule="zero", out=dt)
        kw = dict(alpha=0.2, relu=True, heads=heads, fill_dead_rows=False)
        # two stages (the side outputs ask for them): stage B walks the schedule
        D, E, S = _three_ways(lambda: ops.gat_aggregate(A, Wh, att, want_edge_outputs=True, **kw))
        _close(D, ref["D"], dt)
        # one walk, wherever it applies (elsewhere this is the two-stage form without side outputs)
        with _lib.tuning(SGX_GAT_FUSED="2"):
            (Df,) = _three_ways(lambda: (ops.gat_aggregate(A, Wh, att, **kw),))
        _close(Df, ref["D"], dt)
