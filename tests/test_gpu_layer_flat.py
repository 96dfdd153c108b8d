"""The layers on the entry-split schedule (sgx_layer_desc.schedule_adj = SGX_SCHEDULE_FLAT; ops.layer_forward(schedule="flat")
or an adjacency marked with_facts(flat=True)): the route (ops.layer_schedule), the bit rule -- the layer equals its X.W stage
call followed by ops.spmm / ops.gat_aggregate(schedule="flat"), statistics included -- inside the float64 bounds of
_spmm_acc_ref / _gat_ref, writes that stay inside D and the workspace, a recorded layer replayed on another matrix of the
same capacity, the unmarked call bit-equal to the direct sgx_layer_forward it made before, a whole FPYNQ_GAT training step
on a flat-marked adjacency with a hub row and a hub column (no plan built, nothing synchronised, gradients inside
_layer_grad_ref's bound), and the transpose of a flat-marked matrix.

The layer graph (T = sgx_spmm_flat_chunk() = 256; 40 rows, 700 columns): row 1 of 600 entries from entry 5 on -- it crosses
the chunk ends at 256 and 512 --, row 2 ending exactly on entry 768 = 3 T, six empty rows, a row whose values are all
negative (dead under the GAT mask), short random rows; a fifth of the other values are negative (masked)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _gat_ref as G
import _layer_grad_ref as LG
import _spmm_acc_ref as SA
import _spmm_flat_ref as F

pytestmark = pytest.mark.gpu
TDT = {"f16": torch.float16, "f32": torch.float32}
N_COLS, M_FEA, ALPHA = 700, 20, 0.2
LONG, ON_END, DEAD = 1, 2, 10
SENTINEL = -77.0
# error / magnitude bound of the gradients: test_gpu_layer_grad.py's figures and reasoning (fp32 sums stay below ~4e-7 of the
# bound for grad_input / grad_weights, ~2e-9 for grad_attention whose bound adds magnitudes that cancel)
GRAD_TOL = dict(grad_input=1e-5, grad_weights=1e-5, grad_attention=1e-7)


@functools.lru_cache(maxsize=None)
def T():
    from sgracex1_amd import _lib
    return _lib.lib.sgx_spmm_flat_chunk()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def layer_degrees():
    t = T()
    deg = [5, 600, 3 * t - 605] + [0] * 6 + [7, 9] + list(np.random.default_rng(5).poisson(6.0, 29))
    rp = np.concatenate([[0], np.cumsum(deg)])
    assert rp[LONG] // t == 0 and (rp[LONG + 1] - 1) // t == 2 and rp[ON_END + 1] == 3 * t and len(deg) == 40
    return deg


@functools.lru_cache(maxsize=None)
def layer_graph(dt, seed=0, deg=None):
    """(rowptr, col, val float64 of stored values) on the CPU"""
    rp, ci, va = F.build(layer_degrees() if deg is None else list(deg), N_COLS, dt, seed=seed)
    if deg is None:
        va[rp[DEAD]:rp[DEAD + 1]] = -np.abs(va[rp[DEAD]:rp[DEAD + 1]])
    return rp, ci, va


def csr_of(g, dt, capacity=None, **facts):
    from sgracex1_amd import ops
    rp, ci, va = g
    cap = len(ci) if capacity is None else capacity
    col = torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda")
    val = torch.zeros(max(cap, 1), dtype=TDT[dt], device="cuda")
    col[:len(ci)] = torch.as_tensor(ci)
    val[:len(ci)] = torch.as_tensor(va).to(TDT[dt])
    A = ops.Csr(torch.as_tensor(rp, dtype=torch.int32, device="cuda"), col[:cap], val[:cap], N_COLS)
    return A.with_facts(**facts) if facts else A


@functools.lru_cache(maxsize=None)
def operands(dt, P, seed=0):
    """X dense [N_COLS, M_FEA] (60 % zeros), its CSR, Wt [P, M_FEA], the attention vector [2 P]; values the type holds"""
    from sgracex1_amd import ops
    rng = np.random.default_rng(100 + P + seed)
    X = SA.rounded((rng.random((N_COLS, M_FEA)) - 0.3) * (rng.random((N_COLS, M_FEA)) < 0.4), dt)
    Wt = SA.rounded((rng.random((P, M_FEA)) * 2 - 1) / np.sqrt(M_FEA), dt)
    att = SA.rounded(rng.standard_normal(2 * P) / np.sqrt(P), dt)
    Xd = torch.as_tensor(X).to(TDT[dt]).cuda()
    return Xd, ops.Csr.from_dense(Xd), torch.as_tensor(Wt).to(TDT[dt]).cuda(), torch.as_tensor(att).to(TDT[dt]).cuda()


def stage_h(fea, Wt):
    """the X.W stage call on its own, into rows of the layer's pitch: sgx_xw_dense, or sgx_transpose + sgx_xw_sparse"""
    from sgracex1_amd import ops
    P = Wt.shape[0]
    ldh = ops.table_pitch(P, Wt.element_size())
    if not isinstance(fea, ops.Csr):
        return ops.xw_dense(fea, Wt, ldh=ldh)
    W = ops.transpose(Wt, ldo=ldh)
    H = torch.zeros((fea.n_rows, ldh), dtype=Wt.dtype, device="cuda")
    return ops.xw_sparse(fea, W[:, :P], out=H[:, :P])


def features(dt, P, sparse):
    Xd, Xc, Wt, att = operands(dt, P)
    return (Xc if sparse else Xd), Wt, att


CASES = [(dt, P, sparse, relu) for dt in ("f16", "f32") for P in (3, 64) for sparse in (False, True) for relu in (0, 1)]


# ---- 1. the route ---------------------------------------------------------------------------------------------------------------

def test_route():
    from sgracex1_amd import ops
    for dt in ("f16", "f32"):
        for sparse in (False, True):
            fea, Wt, att = features(dt, 64, sparse)
            plain, marked = csr_of(layer_graph(dt), dt), csr_of(layer_graph(dt), dt, flat=True)
            for kw in (dict(), dict(gat_attention=att, fill_dead_rows=True)):
                assert ops.layer_schedule(plain, fea, Wt, **kw) == 0
                assert ops.layer_schedule(plain, fea, Wt, schedule="flat", **kw) == 2
                assert ops.layer_schedule(marked, fea, Wt, **kw) == 2
            # what the entry-split calls do not have: a flat-marked matrix runs as without the fact
            assert ops.layer_schedule(marked, fea, Wt, gat_attention=att, fill_dead_rows=True, want_edge_outputs=True) == 0
            assert ops.layer_schedule(marked, fea, Wt, acc_mode=ops.SGX_ACC_REF_HALF) == 0
            assert plain._plan is None and marked._plan is None
    big = csr_of(training_graph(), "f32")                                # 8192 entries and more: planned today
    X = torch.zeros((big.n_cols, M_FEA), device="cuda")
    Wt = torch.zeros((16, M_FEA), device="cuda")
    assert big.wants_plan and ops.layer_schedule(big, X, Wt) == 1 and ops.layer_schedule(big, X, Wt, schedule="flat") == 2
    assert ops.layer_schedule(big, X, Wt, use_plan=False) == 0


# ---- 2. the bit rule, GCN ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,P,sparse,relu", CASES)
def test_bit_rule_gcn(dt, P, sparse, relu):
    from sgracex1_amd import ops
    g = layer_graph(dt)
    fea, Wt, _ = features(dt, P, sparse)
    H = stage_h(fea, Wt)
    want = ops.spmm(csr_of(g, dt), H, relu=bool(relu), n_feat=P, schedule="flat")
    by_keyword = ops.layer_forward(csr_of(g, dt), fea, Wt, relu=bool(relu), schedule="flat")
    by_fact = ops.layer_forward(csr_of(g, dt, flat=True), fea, Wt, relu=bool(relu))
    assert torch.equal(bits(by_keyword), bits(want)) and torch.equal(bits(by_fact), bits(want))
    s, scale, n = SA.one_pass(g, H.double().cpu().numpy())
    ref, bound = SA.finished(s, SA.partial_bound(n, scale), dt, relu)
    SA.assert_within(f"gcn {dt} P={P} sparse={sparse} relu={relu}", by_keyword.double().cpu().numpy(), ref, bound)
    if sparse:
        # a flat-marked feature CSR: the X.W stage as an entry-split aggregation over W, the layer the two stage calls
        Xf = ops.Csr(fea.rowptr, fea.col, fea.val, fea.n_cols).with_facts(flat=True)
        ldh = ops.table_pitch(P, Wt.element_size())
        Hf = torch.zeros((N_COLS, ldh), dtype=Wt.dtype, device="cuda")
        ops.spmm(Xf, ops.transpose(Wt, ldo=ldh), n_feat=P, out=Hf[:, :P], schedule="flat")
        got = ops.layer_forward(csr_of(g, dt, flat=True), Xf, Wt, relu=bool(relu))
        assert torch.equal(bits(got), bits(ops.spmm(csr_of(g, dt), Hf, relu=bool(relu), n_feat=P, schedule="flat")))
        assert ops.layer_schedule(csr_of(g, dt, flat=True), Xf, Wt) == 2 and Xf._plan is None
        s, scale, n = SA.one_pass(g, Hf[:, :P].double().cpu().numpy())
        ref, bound = SA.finished(s, SA.partial_bound(n, scale), dt, relu)
        SA.assert_within(f"gcn, flat X.W {dt} P={P} relu={relu}", got.double().cpu().numpy(), ref, bound)


# ---- 3. the bit rule, attention --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,P,sparse,relu", CASES)
def test_bit_rule_attention(dt, P, sparse, relu):
    """the three dead-row rules a layer can ask for: decided from the adjacency (it has a dead row: the mean row), the mean
    row, zero"""
    from sgracex1_amd import ops
    g = layer_graph(dt)
    rp, ci, va = g
    fea, Wt, att = features(dt, P, sparse)
    H = stage_h(fea, Wt)
    gd = dict(rowptr=rp.astype(np.int64), col=ci.astype(np.int64), val=va, Wh=H.double().cpu().numpy(),
              att=att.double().cpu().numpy(), n_rows=len(rp) - 1, n_cols=N_COLS, names={})
    for rule in (None, True, False):
        what = f"gat {dt} P={P} sparse={sparse} relu={relu} fill={rule}"
        want, wstats = ops.gat_aggregate(csr_of(g, dt), H, att, alpha=ALPHA, relu=bool(relu), fill_dead_rows=rule,
                                         want_row_stats=True, schedule="flat")
        got, stats = ops.layer_forward(csr_of(g, dt), fea, Wt, relu=bool(relu), gat_attention=att, alpha=ALPHA, want_row_stats=True,
                                       fill_dead_rows=rule, schedule="flat")
        assert torch.equal(bits(got), bits(want)), what
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(stats.tensors(), wstats.tensors())), what
        plain = ops.layer_forward(csr_of(g, dt, flat=True), fea, Wt, relu=bool(relu), gat_attention=att, alpha=ALPHA,
                                  fill_dead_rows=rule)
        assert torch.equal(bits(plain), bits(want)), what                # the fact, and no statistics: the same D
        ref = G.forward(gd, 1, alpha=ALPHA, relu=bool(relu), dead_rule="zero" if rule is False else "mean", out=dt)
        assert ref["dead"][DEAD] and ref["dead"].sum() >= 7              # the masked row and the empty ones
        G.check(what, got.double().cpu().numpy(), ref["D"], ref["bD"], np.arange(len(rp) - 1), {})


# ---- 4. writes stay in bounds, runs repeat -----------------------------------------------------------------------------------------

def direct_layer(A, fea, Wt, relu=0, att=None, fill=0, flat=False, plan=None, guard=False):
    """sgx_layer_forward on a descriptor built here, into a NaN-filled D between two sentinel rows and a workspace of its
    own between two 256-byte guard bands -> (D with its sentinel rows, the workspace with its bands, the bytes between)"""
    from sgracex1_amd import _lib, ops
    P, M = Wt.shape
    d = _lib.LayerDesc(gemm_mode=0 if isinstance(fea, ops.Csr) else 1, relu=relu, gat_mode=int(att is not None), N_adj=A.n_rows,
                       M_adj=A.n_cols, M_fea=M, P_w=P, dtype=ops.dtype_code(Wt.dtype), spmm_block=1, fea_threads=1, adj_threads=1,
                       gat_fill_dead_rows=fill, alpha=ALPHA, B=Wt.data_ptr(), rowPtr_adj=A.rowptr.data_ptr(),
                       columnIndex_adj=A.col.data_ptr(), values_adj=A.val.data_ptr())
    if isinstance(fea, ops.Csr):
        d.rowPtr_fea, d.columnIndex_fea, d.values_fea = fea.rowptr.data_ptr(), fea.col.data_ptr(), fea.val.data_ptr()
    else:
        d.values_fea = fea.data_ptr()
    if att is not None:
        d.attention, d.gat_heads = att.data_ptr(), 1
    if flat:
        d.schedule_adj, d.nnz_adj = _lib.SGX_SCHEDULE_FLAT, A.nnz
    if plan is not None:
        d.plan_adj = plan.handle
    D = torch.full((A.n_rows + 2, P), float("nan"), dtype=Wt.dtype, device="cuda")
    D[0], D[-1] = SENTINEL, SENTINEL
    d.D = D[1:].data_ptr()
    nbytes = _lib.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
    ws = torch.full((nbytes + 768,), 0xA5, dtype=torch.uint8, device="cuda")
    off = (-ws.data_ptr()) % 256 + 256
    d.workspace, d.workspace_bytes = ws.data_ptr() + off, nbytes
    ops.check(_lib.lib.sgx_layer_forward(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "sgx_layer_forward")
    return D, ws, (off, nbytes)


@pytest.mark.parametrize("dt,P,sparse", [(dt, P, sp) for dt in ("f16", "f32") for P in (3, 64) for sp in (False, True)])
def test_writes_stay_in_bounds_and_runs_repeat(dt, P, sparse):
    from sgracex1_amd import ops
    A = csr_of(layer_graph(dt), dt)
    fea, Wt, att = features(dt, P, sparse)
    for a, fill in ((None, 0), (att, 0), (att, 1)):
        what = f"{dt} P={P} sparse={sparse} gat={a is not None} fill={fill}"
        D, ws, (off, nbytes) = direct_layer(A, fea, Wt, relu=1, att=a, fill=fill, flat=True)
        again = direct_layer(A, fea, Wt, relu=1, att=a, fill=fill, flat=True)[0]
        assert nbytes > 0 and (D[0] == SENTINEL).all() and (D[-1] == SENTINEL).all(), f"{what}: a store outside the rows of D"
        assert not torch.isnan(D[1:-1]).any(), f"{what}: a row of D was not written"
        assert (ws[:off] == 0xA5).all() and (ws[off + nbytes:] == 0xA5).all(), f"{what}: a store outside the workspace"
        assert torch.equal(bits(D), bits(again)), f"{what}: two runs differ"
        kw = dict(gat_attention=a, alpha=ALPHA, fill_dead_rows=bool(fill)) if a is not None else {}
        assert torch.equal(bits(D[1:-1]), bits(ops.layer_forward(A, fea, Wt, relu=True, schedule="flat", **kw))), what


# ---- 5. record and replay ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gat", [False, True])
def test_recorded_layer_replays_on_another_matrix(gat):
    """recorded at a capacity of 3 T entries on a side stream after a warm-up, under sync-debug "error"; then rowptr, col and
    val are overwritten in place with a matrix of another long row and fewer entries: the replay equals the eager layer"""
    from sgracex1_amd import ops
    t, dt = T(), "f32"
    cap = 3 * t
    first = layer_graph(dt, 1, tuple([5, 600, 0, 9] + [3] * 36))
    second = layer_graph(dt, 2, tuple([11] * 20 + [0, 0, 300, 40] + [2] * 16))
    assert len(first[1]) <= cap and len(second[1]) < len(first[1]) and len(second[0]) == len(first[0])
    fea, Wt, att = features(dt, 64, False)
    kw = dict(gat_attention=att, alpha=ALPHA, fill_dead_rows=True) if gat else {}
    A = csr_of(first, dt, capacity=cap)
    out = torch.empty((A.n_rows, 64), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.layer_forward(A, fea, Wt, relu=True, out=out, schedule="flat", **kw)         # warm-up: sizes the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_first = out.clone()
    recorded = torch.cuda.CUDAGraph()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.graph(recorded, stream=side):
            ops.layer_forward(A, fea, Wt, relu=True, out=out, schedule="flat", **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert A._plan is None
    out.fill_(SENTINEL)
    recorded.replay()
    assert torch.equal(bits(out), bits(eager_first))
    rp2, ci2, va2 = second
    A.rowptr.copy_(torch.as_tensor(rp2, dtype=torch.int32))
    A.col[:len(ci2)] = torch.as_tensor(ci2).cuda()
    A.col[len(ci2):] = 1 << 30                                           # what lies behind the new end is never read
    A.val[:len(ci2)] = torch.as_tensor(va2).float().cuda()
    A.val[len(ci2):] = float("nan")
    out.fill_(SENTINEL)
    recorded.replay()
    replayed = out.clone()
    eager = ops.layer_forward(csr_of(second, dt, capacity=cap), fea, Wt, relu=True, schedule="flat", **kw)
    assert torch.equal(bits(replayed), bits(eager))


# ---- 6. the unmarked call is unchanged -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("gat", [False, True])
def test_unmarked_call_is_unchanged(gat):
    from sgracex1_amd import ops
    for dt, P, sparse in (("f16", 64, False), ("f16", 3, True), ("f32", 64, True)):
        A = csr_of(layer_graph(dt), dt)
        fea, Wt, att = features(dt, P, sparse)
        kw = dict(gat_attention=att, alpha=ALPHA, fill_dead_rows=True) if gat else {}
        got = ops.layer_forward(A, fea, Wt, relu=True, **kw)
        assert not A._flat and A._plan is None                           # a small matrix: no plan, as before
        D, _, _ = direct_layer(A, fea, Wt, relu=1, att=att if gat else None, fill=1)
        assert torch.equal(bits(got), bits(D[1:-1])), (dt, P, sparse)
    big = csr_of(training_graph(), "f32")                                # from 8192 entries on: the plan it chose before
    X = operands("f32", 16, seed=3)[0]
    Wt, att = operands("f32", 16, seed=3)[2:]
    kw = dict(gat_attention=att, alpha=ALPHA, fill_dead_rows=True) if gat else {}
    got = ops.layer_forward(big, X, Wt, relu=True, **kw)
    assert (getattr(big, "_gat_plan", None) if gat else big._plan) is not None
    D, _, _ = direct_layer(big, X, Wt, relu=1, att=att if gat else None, fill=1, plan=big.gat_plan if gat else big.plan)
    assert torch.equal(bits(got), bits(D[1:-1]))


# ---- 7. a training step ----------------------------------------------------------------------------------------------------------

HUB = 600


@functools.lru_cache(maxsize=None)
def training_graph():
    """square, 700 nodes, at least 8192 entries: row 0 holds HUB entries, column 1 stands in HUB rows; a row of negative
    values (dead under the mask), an empty row, a fifth of the values negative (masked)"""
    rng = np.random.default_rng(17)
    n = N_COLS
    rows = []
    for i in range(n):
        k = HUB if i == 0 else (0 if i == 5 else 11)
        c = set(rng.choice(n, k, replace=False).tolist())
        if 2 <= i < 2 + HUB:
            c.add(1)
        rows.append(np.array(sorted(c), np.int32))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows)
    va = rng.random(len(ci)) * 2.0 - 0.4
    va[va == 0] = 0.5
    va[rp[7]:rp[8]] = -np.abs(va[rp[7]:rp[8]])
    assert len(ci) >= 8192 and rp[1] == HUB and (ci == 1).sum() >= HUB
    return rp, ci, SA.rounded(va, "f32")


def softmax_reference(rp, ci, va, X, W, att, alpha):
    """E, S per stored entry and the dead rows, in float64 from the formulas (SG.py:634-661)"""
    rowptr = torch.as_tensor(rp, dtype=torch.int64, device="cuda")
    col, val = torch.as_tensor(ci, dtype=torch.int64, device="cuda"), torch.as_tensor(va, device="cuda").double()
    n = rowptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), rowptr[1:] - rowptr[:-1])
    Wh = X.double() @ W.double()
    P = W.shape[1]
    z = (Wh @ att.double()[:P, 0])[row] + (Wh @ att.double()[P:, 0])[col]
    E = torch.where(z > 0, z, alpha * z)
    live = val > 0
    m = torch.full((n,), -float("inf"), dtype=torch.float64, device="cuda").scatter_reduce(0, row[live], E[live], "amax")
    p = torch.where(live, torch.exp(E - torch.where(live, m[row], torch.zeros_like(E))), torch.zeros_like(E))
    l = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, row, p)
    dead = l == 0
    return E, torch.where(dead[row], torch.zeros_like(p), p / l[row].clamp_min(1e-300)), dead


@pytest.mark.parametrize("gat", [1, 0])
def test_training_step_on_a_flat_marked_adjacency(gat, monkeypatch):
    """forward + backward of GATConv_SGRACE under sync-debug "error" with no plan built anywhere (torch's sync-debug mode does
    not see a read-back made inside the library, so the plans are counted as well: without the fact carried to the
    attention matrix P, ops.spmm(P, g) builds one for a matrix of 8192 entries and more)"""
    from sgracex1_amd import config, ops, sgrace
    rp, ci, va = training_graph()
    M, P = 24, 16
    rng = torch.Generator(device="cuda")
    rng.manual_seed(5)
    X = (torch.rand((N_COLS, M), generator=rng, device="cuda") - 0.3).half().float()
    W = ((torch.rand((M, P), generator=rng, device="cuda") * 2 - 1) / M ** 0.5).half().float()
    att = ((torch.rand((2 * P, 1), generator=rng, device="cuda") * 2 - 1) * 0.7).half().float()
    Gr = torch.randn((N_COLS, P), generator=rng, device="cuda")
    E, S, dead = softmax_reference(rp, ci, va, X, W, att, ALPHA)
    assert bool(dead[5]) and bool(dead[7]) and int(dead.sum()) == 2
    A = csr_of((rp, ci, va), "f32", dead_row_mask=dead, has_dead_rows=True, flat=True)
    built = []
    plan_init = ops.Plan.__init__
    monkeypatch.setattr(ops.Plan, "__init__", lambda self, *a, **k: (built.append(a), plan_init(self, *a, **k))[1])
    old = config.snapshot()
    try:
        config.acc, config.compute_attention, config.device, config.float_type = 1, gat, "cuda", np.float32
        config.fake_quantization, config.hardware_quantize, config.accb, config.gat_edge_outputs = 0, 0, 0, 1
        sgrace.init_SGRACE()
        layer = sgrace.GATConv_SGRACE(M, P).to("cuda")
        with torch.no_grad():
            layer.weight.copy_(W), layer.attention.copy_(att)
        x = X.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = layer(gat, 1, 0, x, None, A.val, A)
            out.backward(Gr)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
    assert not built and A._plan is None, f"{len(built)} plans were built"
    AT = A._transpose_pattern[0] if gat else None
    assert AT is None or (AT._flat and AT._plan is None)
    grads, bounds = LG.edges(torch.as_tensor(rp).cuda(), torch.as_tensor(ci).cuda(), torch.as_tensor(va).cuda(), X, W, Gr,
                             gat=bool(gat), E=E, S=S, dead=dead, alpha=ALPHA)
    got = dict(grad_input=x.grad, grad_weights=layer.weight.grad)
    if gat:
        got["grad_attention"] = layer.attention.grad
    else:
        assert not layer.attention.grad.any()
    figures = LG.check(got, grads, bounds, GRAD_TOL, ("flat training step", gat))
    print("layer_flat training step", gat, {k: f"{v:.2e}" for k, v in figures.items()})


# ---- 8. the transpose --------------------------------------------------------------------------------------------------------------

def test_transpose_of_a_flat_marked_matrix():
    from sgracex1_amd import ops
    g = training_graph()
    plain = ops.csr_transpose(csr_of(g, "f32"), return_order=True)
    A = csr_of(g, "f32", flat=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        Tm, order = ops.csr_transpose(A, return_order=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    deg = Tm.rowptr[1:] - Tm.rowptr[:-1]
    assert int(deg[1]) >= HUB                                            # the hub column is a long row of the transpose
    assert Tm._flat and Tm._plan is None and not Tm.wants_plan and A._plan is None
    assert not plain[0]._flat
    assert torch.equal(Tm.rowptr, plain[0].rowptr) and torch.equal(Tm.col, plain[0].col) and torch.equal(order, plain[1])
    assert torch.equal(bits(Tm.val), bits(plain[0].val))
    # a feature matrix transposed (a handful of long rows) builds a plan today, and none when it is flat-marked
    Xc = operands("f32", 64)[1]
    wide = ops.Csr(Xc.rowptr, Xc.col, Xc.val, Xc.n_cols)
    assert ops.csr_transpose(wide)._plan is not None
    assert ops.csr_transpose(ops.Csr(Xc.rowptr, Xc.col, Xc.val, Xc.n_cols).with_facts(flat=True))._plan is None
