"""GAT from row softmax statistics (sgx_gat_stats) instead of the per-edge outputs E and S: the forward that delivers
them, the E / S formed again from them, the backward edge pass that reads them, and the SGRACE layer trained that way
(config.gat_edge_outputs = 0) -- against the float64 restatements of tests/_gat_ref.py and tests/_layer_grad_ref.py."""
import numpy as np
import pytest
import torch

import _gat_ref as R
import _layer_grad_ref as LR

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")

DTYPES = {"f16": torch.float16, "f32": torch.float32}
SHAPES = [(1, 64), (8, 32), (1, 256)]                    # heads x columns per head
GRAPHS = {"adversarial": R.adversarial_graph, "plain": R.plain_graph}
MAX_LEFT_OUT = 0.005                                     # share of live entries whose slope the reference cannot tell


class Case:
    """One graph of one element type and head layout on the device."""

    def __init__(self, kind, dt, heads, f_head):
        g = self.g = GRAPHS[kind](dt, heads, f_head, seed=100 * heads + f_head)
        tdt = DTYPES[dt]
        self.dt, self.heads, self.f_head = dt, heads, f_head
        self.rowptr = torch.as_tensor(g["rowptr"], dtype=torch.int32, device=dev)
        self.col = torch.as_tensor(g["col"], dtype=torch.int32, device=dev)
        self.val = torch.as_tensor(g["val"]).to(tdt).to(dev)
        self.Wh = torch.as_tensor(g["Wh"]).to(tdt).to(dev)
        self.att = torch.as_tensor(g["att"]).to(tdt).to(dev)
        rng = np.random.default_rng(heads + f_head)
        self.fill_row = R._round(rng.standard_normal(heads * f_head), "f32")
        self.fill_t = torch.as_tensor(self.fill_row, dtype=torch.float32, device=dev)
        self.n_nodes = g["n_cols"] + 13
        self._refs = {}

    def csr(self):
        from sgracex1_amd import ops
        A = ops.Csr(self.rowptr, self.col, self.val, self.g["n_cols"])
        assert A.wants_plan                              # (use_plan decides: the graphs are large enough to get one)
        return A

    def ref(self, rule):
        if rule not in self._refs:
            self._refs[rule] = R.forward(self.g, self.heads, dead_rule=rule, fill_row=self.fill_row, n_nodes=self.n_nodes,
                                         out=self.dt)
        return self._refs[rule]

    def kwargs(self, rule, plan):
        kw = dict(alpha=0.2, heads=self.heads, use_plan=plan)
        if rule == "fill":
            kw.update(fill_row=self.fill_t, n_nodes=self.n_nodes)
        else:
            kw.update(fill_dead_rows=rule == "mean")
        return kw

    def dead_weight(self, rule):
        return {"zero": 0.0, "mean": 1.0 / self.g["n_cols"], "fill": 1.0 / self.n_nodes}[rule]


@pytest.fixture(scope="module")
def cases():
    store = {}

    def get(*key):
        if key not in store:
            store[key] = Case(*key)
        return store[key]
    return get


@pytest.mark.parametrize("plan", [True, False], ids=["plan", "noplan"])
@pytest.mark.parametrize("rule", ["zero", "mean", "fill"])
@pytest.mark.parametrize("heads,f_head", SHAPES)
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", list(GRAPHS))
def test_forward_with_statistics(cases, kind, dt, heads, f_head, rule, plan):
    """D inside bD and bit-equal to the call without side outputs; E, S formed from the statistics inside bE, bS;
    row_sum == 0 exactly on the reference's dead rows (row_max too)."""
    from sgracex1_amd import ops
    c = cases(kind, dt, heads, f_head)
    A, kw = c.csr(), c.kwargs(rule, plan)
    D, stats = ops.gat_aggregate(A, c.Wh, c.att, want_row_stats=True, **kw)
    D_plain = ops.gat_aggregate(A, c.Wh, c.att, **kw)
    assert torch.equal(D, D_plain), "D differs from the aggregate without side outputs"
    E, S = ops.gat_edge_outputs(A, stats, alpha=0.2, dead_weight=c.dead_weight(rule))
    for name, t in (("D", D), ("E", E), ("S", S), *zip(("score_row", "score_col", "row_max", "row_sum"), stats.tensors())):
        assert torch.isfinite(t).all(), f"{name}: not finite"
    ref = c.ref(rule)
    R.check_forward({"D": D.double().cpu().numpy(), "E": E.double().cpu().numpy(), "S": S.double().cpu().numpy()}, ref,
                    c.g["names"])
    dead = torch.as_tensor(ref["dead"], device=dev)
    l0 = stats.row_sum.reshape(c.g["n_rows"], heads) == 0
    assert torch.equal(l0, dead[:, None].expand(-1, heads)), "row_sum == 0 is not exactly the dead rows"
    assert not stats.row_max.reshape(c.g["n_rows"], heads)[dead].any()
    D2, stats2 = ops.gat_aggregate(A, c.Wh, c.att, want_row_stats=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(stats.tensors(), stats2.tensors())), "not the same bits on a second run"


@pytest.mark.parametrize("dt", list(DTYPES))
def test_the_statistics_call_takes_the_one_walk(cases, dt):
    """8 heads of 32 columns with a plan: the aggregate without side outputs runs as one walk (gat_fused.hip), whose
    neighbour scores and exponentials differ in the last bits from the two stages'.  The statistics call gives the one
    walk's D by default and the two stages' D when the one walk is switched off -- it follows the same choice."""
    from sgracex1_amd import _lib, ops
    c = cases("adversarial", dt, 8, 32)
    A, kw = c.csr(), c.kwargs("zero", True)
    D_walk = ops.gat_aggregate(A, c.Wh, c.att, **kw)
    D_stats, _ = ops.gat_aggregate(A, c.Wh, c.att, want_row_stats=True, **kw)
    with _lib.tuning(SGX_GAT_FUSED="0"):
        D_two = ops.gat_aggregate(A, c.Wh, c.att, **kw)
        D_stats_two, _ = ops.gat_aggregate(A, c.Wh, c.att, want_row_stats=True, **kw)
    assert not torch.equal(D_walk, D_two), "the two forms gave the same bits: the case does not tell them apart"
    assert torch.equal(D_stats, D_walk) and torch.equal(D_stats_two, D_two)


@pytest.mark.parametrize("rule", ["zero", "mean"])
@pytest.mark.parametrize("f_head", [64, 256])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", list(GRAPHS))
def test_backward_edges_from_statistics(cases, kind, dt, f_head, rule):
    """sg, g1 and S_out of sgx_gat_backward_edges_stats against backward_edges() fed the reference's own float64 E, S.

    Bound.  The kernel's weights w = S + dS (|dS_e| <= bS_e, the forward restatement's bound: the statistics' E and S
    are the forward's own) enter sg_e = (w_e d_e - w_e rs_i) slope_e with rs_i = sum_row w d.  To first order in dS
        d(sg_e) = dS_e (d_e - rs_i) - S_e sum_row(dS d)
    so, next to backward_edges' own bound b_sg for exact inputs,
        |sg_e - ref| <= b_sg_e + bS_e (|d_e| + |rs_i|) + S_e sum_row(bS |d|)
    (the slope is at most 1 in magnitude), and g1_i, the row sum of sg, within b_g1_i plus the row sum of the added term.
    On a dead row of the "mean" rule rs_i = G_i . mean(Wh) is not formed from the weights; the term stays as an upper
    bound.  The slope is a step in E_e: where |E_e| <= bE_e the reference cannot tell its sign, so those entries are left
    out together with their row's g1 -- at most 0.5 % of the live entries, asserted."""
    from sgracex1_amd import ops
    c = cases(kind, dt, 1, f_head)
    A = c.csr()
    _, stats = ops.gat_aggregate(A, c.Wh, c.att, want_row_stats=True, **c.kwargs(rule, True))
    check_backward_from_statistics(c.g, c.ref(rule), A, stats, c.Wh, f_head, rule == "mean", c.dead_weight(rule),
                                   (kind, dt, f_head, rule))


def check_backward_from_statistics(g, ref, A, stats, Wh, f_head, mean_rule, dead_weight, what):
    """The comparison of test_backward_edges_from_statistics on graph g with its forward restatement ref, the adjacency
    A on the device, its statistics and Wh [n_cols, f_head]; returns (G, sg, g1, S_out)."""
    from sgracex1_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(f_head)
    G = torch.randn((g["n_rows"], f_head), generator=gen, device="cuda")
    Whf = Wh.float()
    dead = A.dead_rows if mean_rule else None
    run = lambda: ops.gat_backward_edges_stats(A, stats, G, Whf, alpha=0.2, dead=dead, dead_weight=dead_weight)
    sg, g1, S_out = run()
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((sg, g1, S_out), again)), "not the same bits on a second run"
    dead_np = None if dead is None else dead.cpu().numpy()
    assert dead_np is None or np.array_equal(dead_np, ref["dead"])
    Gn = G.double().cpu().numpy()
    want_sg, want_g1, b_sg, b_g1 = R.backward_edges(g, ref["E"], ref["S"], Gn, g["Wh"], dead=dead_np)
    rowptr, col = g["rowptr"].astype(np.int64), g["col"].astype(np.int64)
    row = ref["row"]
    d = np.einsum("ek,ek->e", Gn[row], g["Wh"][col])
    rs = R._seg(np.add, ref["S"] * d, rowptr, 0.0)
    if dead_np is not None:
        rs = np.where(dead_np, Gn @ g["Wh"].mean(0), rs)
    extra = ref["bS"] * (np.abs(d) + np.abs(rs[row])) + ref["S"] * R._seg(np.add, ref["bS"] * np.abs(d), rowptr, 0.0)[row]
    extra = np.where(ref["live"], extra, 0.0)
    unsure = ref["live"] & (np.abs(ref["E"]) <= ref["bE"])
    n_live = int(ref["live"].sum())
    print("backward_stats", *what, "left out", int(unsure.sum()), "of", n_live, "live entries")
    assert unsure.sum() <= MAX_LEFT_OUT * n_live
    keep_e = ~unsure
    keep_r = R._seg(np.add, unsure.astype(np.int64), rowptr, 0) == 0
    names = g["names"]
    R.check("S_out", S_out.double().cpu().numpy(), ref["S"], ref["bS"], row, names)
    R.check("sg", sg.double().cpu().numpy()[keep_e], want_sg[keep_e], (b_sg + extra)[keep_e], row[keep_e], names)
    b_g1x = b_g1 + R._seg(np.add, extra, rowptr, 0.0)
    R.check("g1", g1.double().cpu().numpy()[keep_r], want_g1[keep_r], b_g1x[keep_r], np.arange(g["n_rows"])[keep_r], names)
    return G, sg, g1, S_out


# ---- the SGRACE layer with config.gat_edge_outputs = 0 -------------------------------------------------------------------

def _masked_csr(n, seed, density):
    from sgracex1_amd import ops
    rowptr, col, val, _rows = LR.masked_graph(n, seed, density=density)
    A = ops.Csr(rowptr.to(torch.int32).to(dev), col.to(torch.int32).to(dev), val.to(dev), n)
    assert bool((A.val <= 0).any()) and bool(LR.dead_rows_of(A.rowptr, A.val).any())
    return A


@pytest.mark.parametrize("dtype,gemm,bits", [(torch.float32, 0, None), (torch.float32, 1, None), (torch.float16, 0, None),
                                             (torch.float16, 1, None), (torch.float32, 1, 8)])
def test_layer_trained_from_statistics(dtype, gemm, bits):
    """GATConv_SGRACE forward + backward with config.gat_edge_outputs = 0 on the masked graph (masked entries, dead rows):
    the output is the layer's output without side outputs bit for bit, and every gradient lies within the layer-gradient
    suite's TOL of the float64 restatement fed the E and S that the E / S ports deliver for the same layer."""
    from test_gpu_layer_grad import TOL, _inputs, _set
    from sgracex1_amd import config, ops, sgrace
    A = _masked_csr(1500, 11, 0.012)
    n, M, P = A.n_rows, 602, 16
    X, W, att, G = _inputs(n, M, P, 5 + 31 * P + M, sparse=gemm == 0)
    old = config.snapshot()
    try:
        _set(1, dtype, bits, 0)
        config.gat_edge_outputs = 0
        qc = sgrace.quant_constants
        layer = sgrace.GATConv_SGRACE(M, P).to(dev)
        with torch.no_grad():
            layer.weight.copy_(W), layer.attention.copy_(att)
        x = X.clone().requires_grad_(True)
        relu = 1 if gemm == 0 else 0
        out = layer(1, gemm, relu, x, None, A.val, A)
        out.backward(G)
        Al = layer._csr
        fea = ops.cached_on(x, ("fea_csr", dtype), lambda: None) if gemm == 0 else x.detach().to(dtype).contiguous()
        kw = dict(relu=relu, alpha=layer.alpha, gat_attention=att.to(dtype).reshape(-1).contiguous(), quant=qc)
        plain = ops.layer_forward(Al, fea, W.t().to(dtype).contiguous(), **kw)
        assert torch.equal(plain.float(), out.detach())
        _o, E, S = ops.layer_forward(Al, fea, W.t().to(dtype).contiguous(), want_edge_outputs=True, **kw)
        masked = Al.val.float() if qc is None else sgrace._fq_unsigned(Al.val.float(), qc.a_s, qc.a_z, qc.w_qbits)
        dead = LR.dead_rows_of(Al.rowptr, masked)
        assert int(dead.sum()) >= (2 if bits is None else 3)
        grads, bounds = LR.edges(Al.rowptr, Al.col, Al.val, x.detach(), W, G, gat=True, E=E, S=S, dead=dead, alpha=layer.alpha)
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
    got = dict(grad_input=x.grad, grad_weights=layer.weight.grad, grad_attention=layer.attention.grad)
    figures = LR.check(got, grads, bounds, TOL, ("lean", gemm, dtype, bits))
    print("lean_layer_grad", gemm, dtype, bits, "dead", int(dead.sum()), {k: f"{v:.2e}" for k, v in figures.items()})


def test_lean_forward_keeps_less_memory():
    """After the forward the lean layer holds the four statistics arrays where the default one holds E and S: at least
    2 nnz 4 - (3 n_rows + n_cols) 4 bytes less, minus 512 B of allocator rounding for each of the six tensors involved.
    (nnz is about 225 n here, so the margin is not in question.)"""
    from test_gpu_layer_grad import _inputs, _set
    from sgracex1_amd import config, sgrace
    A = _masked_csr(1500, 7, 0.15)
    n, M, P = A.n_rows, 64, 16
    assert A.nnz >= 64 * n
    X, W, att, _G = _inputs(n, M, P, 3, sparse=False)
    old = config.snapshot()
    held = {}
    try:
        _set(1, torch.float32, None, 0)
        layer = sgrace.GATConv_SGRACE(M, P).to(dev)
        with torch.no_grad():
            layer.weight.copy_(W), layer.attention.copy_(att)
        for _warm in range(2):                           # workspaces, plans and per-graph caches exist before measuring
            for flag in (1, 0):
                config.gat_edge_outputs = flag
                x = X.clone().requires_grad_(True)
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                out = layer(1, 1, 0, x, None, A.val, A)
                torch.cuda.synchronize()
                held[flag] = torch.cuda.memory_allocated() - before
                del out
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
    saved = held[1] - held[0]
    need = 2 * A.nnz * 4 - (3 * n + A.n_cols) * 4 - 6 * 512
    print("lean_memory", "default holds", held[1], "lean holds", held[0], "saved", saved, "required", need)
    assert saved >= need
