"""Every form of the GAT edge-softmax aggregate -- one pass (gat_one_pass.hip: per row, long rows split, several heads), two stages
(stage A per row for 1 head / 2..64 heads / more than 64 heads (gat_alpha.hip), as a scan in entry order (gat_scan.hip), long rows through
the plan's tasks; stage B (gat_weighted.hip) with and without the degree order's one-step tail), one walk (gat_fused.hip), the scores from
the X.W epilogue (xw_dense.hip) and the dead-row fills -- against the float64 restatement of tests/_gat_ref.py, element
by element inside its stated error bound, on graphs built where softmax code breaks: live scores tens to hundreds apart,
masked entries with the highest scores, the mask's edge values (+0.0, -0.0, tiny negatives, fp16 and fp32 subnormals),
rows without a live entry, rows on each side of the kernels' size steps and long rows whose tasks are masked or sit far
below the row maximum.  Each form is forced by tuning overrides and an explicit plan, and the plan facts that choose it
are asserted.  Also: the same bits twice, finite outputs, and for one head the backward edge pass on that forward's E / S."""
import numpy as np
import pytest
import torch

import _gat_ref as R

pytestmark = pytest.mark.gpu

# (heads, columns per head): the stage-A lane counts 2..64 (heads 2, 3, 6, 12, 16, 32, 64), more than 64 heads (66, 72),
# head blocks of 1 / 2 / 4 / 8, an unaligned table (3 x 50: one column per lane), one-walk heads of 1 to 32 lanes
LAYOUTS = [(1, 8), (1, 64), (1, 100), (1, 256), (2, 64), (3, 50), (4, 32), (6, 16), (12, 8), (16, 8), (32, 4), (64, 2),
           (66, 2), (72, 4)]
DTYPES = {"f16": torch.float16, "f32": torch.float32}

# name: (tuning overrides, plan, entry point, E / S wanted, rule for rows without a live entry)
FORMS = {
    "one_pass": ({}, None, "agg", True, "zero"),
    "one_pass_fill_row": ({}, None, "agg", True, "fill"),
    "one_pass_long": ({"SGX_GAT_ONE_PASS": "1"}, "cut256", "agg", True, "zero"),
    "one_pass_cut64_mean": ({"SGX_GAT_ONE_PASS": "1"}, "cut64", "agg", True, "mean"),
    "rows": ({"SGX_GAT_SCAN": "0"}, "cut256", "agg", True, "zero"),
    "rows_uncut": ({"SGX_GAT_SCAN": "0"}, "uncut", "agg", True, "zero"),
    "rows_weights_from_scores": ({"SGX_GAT_SCAN": "0", "SGX_GAT_FUSED": "0"}, "cut256", "agg", False, "zero"),
    "rows_mean": ({"SGX_GAT_SCAN": "0"}, "cut256", "agg", True, "mean"),
    "rows_fill_row": ({"SGX_GAT_SCAN": "0"}, "cut256", "agg", True, "fill"),
    "scan": ({"SGX_GAT_SCAN": "2"}, "cut256", "agg", True, "zero"),
    "scan_weights_from_scores_mean": ({"SGX_GAT_SCAN": "2", "SGX_GAT_FUSED": "0"}, "cut256", "agg", False, "mean"),
    "ordered_scan": ({}, "ordered", "agg", True, "zero"),
    "ordered_rows_short_tail_mean": ({"SGX_GAT_SCAN": "0"}, "ordered", "agg", True, "mean"),
    "ordered_rows_no_short_tail": ({"SGX_GAT_SCAN": "0", "SGX_SPMM_NO_SHORT_TAIL": "1"}, "ordered", "agg", True, "zero"),
    "fused": ({"SGX_GAT_FUSED": "2"}, "cut256", "agg", False, "zero"),
    "fused_ordered_mean": ({"SGX_GAT_FUSED": "2"}, "ordered", "agg", False, "mean"),
    "fused_ordered_no_short_tail_fill_row": ({"SGX_GAT_FUSED": "2", "SGX_SPMM_NO_SHORT_TAIL": "1"}, "ordered", "agg", False,
                                             "fill"),
    "layer": ({}, "cut256", "layer", True, "mean"),
    "layer_fused": ({"SGX_GAT_FUSED": "2"}, "ordered", "layer", False, "mean"),
    "layer_no_fused_scores": ({"SGX_GAT_NO_FUSED_SCORES": "1", "SGX_GAT_SCAN": "0"}, "cut256", "layer", True, "mean"),
}


class Case:
    """One adversarial graph of one element type and head layout, on the device, with its references."""

    def __init__(self, dt, heads, f_head):
        self.dt, self.heads, self.f_head = dt, heads, f_head
        # (8200 filler rows: a table of 8192 rows and more is what the X.W kernel forms the scores beside)
        g = self.g = R.adversarial_graph(dt, heads, f_head, seed=100 * heads + f_head, n_filler=8200)
        tdt = DTYPES[dt]
        dev = torch.device("cuda")
        self.rowptr = torch.as_tensor(g["rowptr"], dtype=torch.int32, device=dev)
        self.col = torch.as_tensor(g["col"], dtype=torch.int32, device=dev)
        self.val = torch.as_tensor(g["val"]).to(tdt).to(dev)             # (exact: the values are of the type already)
        self.Wh = torch.as_tensor(g["Wh"]).to(tdt).to(dev)
        self.att = torch.as_tensor(g["att"]).to(tdt).to(dev)
        F = heads * f_head
        m = (len(g["protos"]) + 7) // 8 * 8
        X = torch.zeros((g["n_cols"], m), dtype=tdt)
        X[torch.arange(g["n_cols"]), torch.as_tensor(g["proto_id"])] = 1                # one-hot rows: X.W = Wh exactly
        self.X = X.to(dev)
        Wt = torch.zeros((F, m), dtype=torch.float64)
        Wt[:, :len(g["protos"])] = torch.as_tensor(g["protos"]).T
        self.Wt = Wt.to(tdt).contiguous().to(dev)
        rng = np.random.default_rng(heads + f_head)
        self.fill_row = R._round(rng.standard_normal(F), "f32")
        self.fill_t = torch.as_tensor(self.fill_row, dtype=torch.float32, device=dev)
        self.n_nodes = g["n_cols"] + 13
        self._plans, self._refs = {}, {}

    def plan(self, kind):
        from sgracex1_amd import _lib, ops
        if kind not in self._plans:
            # (a matrix under 2^20 entries is cut at 64 whatever the caller asks; the overrides set the cut of a large one)
            thr = {"cut256": 256, "ordered": 256, "cut64": 64, "uncut": 1 << 16}[kind]
            with _lib.tuning(SGX_PLAN_REORDER_BELOW="2" if kind == "ordered" else "0", SGX_PLAN_LONG_THRESHOLD=str(thr),
                             SGX_PLAN_CHUNK=str(thr)):
                p = ops.Plan(self.rowptr, thr, thr)
            assert p.reordered == (kind == "ordered")
            assert (p.long_rows > 0) == (kind != "uncut")
            if kind in ("cut256", "ordered"):
                assert p.export("scan_win").numel() > 0
            self._plans[kind] = p
        return self._plans[kind]

    def csr(self, kind):
        from sgracex1_amd import ops
        A = ops.Csr(self.rowptr, self.col, self.val, self.g["n_cols"])
        if kind is not None:
            A._plan = A._gat_plan = self.plan(kind)
        assert A.nnz >= 8192 and A.has_dead_rows
        return A

    def ref(self, relu, rule):
        key = (relu, rule)
        if key not in self._refs:
            self._refs[key] = R.forward(self.g, self.heads, relu=relu, dead_rule=rule, fill_row=self.fill_row,
                                        n_nodes=self.n_nodes, out=self.dt)
        return self._refs[key]

    def run(self, A, entry, want_es, rule, relu):
        from sgracex1_amd import ops
        if entry == "layer":
            out = ops.layer_forward(A, self.X, self.Wt, relu=relu, gat_attention=self.att, alpha=0.2,
                                    want_edge_outputs=want_es, gat_heads=self.heads)
        else:
            kw = dict(alpha=0.2, relu=relu, want_edge_outputs=want_es, heads=self.heads, use_plan=A._plan is not None)
            if rule == "fill":
                kw.update(fill_row=self.fill_t, n_nodes=self.n_nodes)
            else:
                kw.update(fill_dead_rows=rule == "mean")
            out = ops.gat_aggregate(A, self.Wh, self.att, **kw)
        D, E, S = out if want_es else (out, None, None)
        return {k: v for k, v in (("D", D), ("E", E), ("S", S)) if v is not None}


@pytest.fixture(scope="module")
def cases():
    store = {}

    def get(dt, heads, f_head):
        if (dt, heads, f_head) not in store:
            store[(dt, heads, f_head)] = Case(dt, heads, f_head)
        return store[(dt, heads, f_head)]
    return get


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dt,heads,f_head", [(dt, h, f) for dt in DTYPES for h, f in LAYOUTS])
def test_gat_form_against_the_float64_restatement(cases, dt, heads, f_head, form):
    from sgracex1_amd import _lib, ops
    c = cases(dt, heads, f_head)
    tune, plan_kind, entry, want_es, rule = FORMS[form]
    relu = rule != "zero"
    A = c.csr(plan_kind)
    with _lib.tuning(**tune):
        got = c.run(A, entry, want_es, rule, relu)
        again = c.run(A, entry, want_es, rule, relu)
    for k, v in got.items():
        assert torch.isfinite(v).all(), f"{k}: not finite"
        assert torch.equal(v, again[k]), f"{k}: not the same bits on a second run"
    ref = c.ref(relu, rule)
    R.check_forward({k: v.double().cpu().numpy() for k, v in got.items()}, ref, c.g["names"])
    if heads == 1 and want_es and entry == "agg" and rule != "fill":
        # the backward edge pass on this forward's own E / S; a dead row of the "mean" rule has a uniform softmax
        gen = torch.Generator(device="cuda")
        gen.manual_seed(f_head)
        G = torch.randn((c.g["n_rows"], f_head), generator=gen, device="cuda")
        Whf = c.Wh.float()
        dead = A.dead_rows if rule == "mean" else None
        sg, g1 = ops.gat_backward_edges(A, got["E"], got["S"], G, Whf, alpha=0.2, dead=dead)
        sg2, g12 = ops.gat_backward_edges(A, got["E"], got["S"], G, Whf, alpha=0.2, dead=dead)
        assert torch.equal(sg, sg2) and torch.equal(g1, g12)
        want = R.backward_edges(c.g, got["E"].cpu().numpy(), got["S"].cpu().numpy(), G.cpu().numpy(), c.g["Wh"],
                                dead=None if dead is None else dead.cpu().numpy())
        names = c.g["names"]
        R.check("sg", sg.double().cpu().numpy(), want[0], want[2], R.rows_of(c.g["rowptr"]), names)
        R.check("g1", g1.double().cpu().numpy(), want[1], want[3], np.arange(c.g["n_rows"]), names)
