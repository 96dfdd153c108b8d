"""sgx_layer_backward on the entry-split schedules (sgx_layer_grad_desc.schedule_adj / _fea / _xt = SGX_SCHEDULE_FLAT;
ops.layer_backward on flat-marked matrices): the route (sgx_layer_backward_schedule), THE BIT RULE -- every output equals
the named stage calls composed on the same operands and capacities: the X.W stage, the edge pass, sgx_gat_attention_grad_flat,
sgx_spmm_csr_flat, sgx_xw_dense / sgx_xt_g --, the float64 restatement of the reference's backward (_layer_grad_ref) inside
test_gpu_layer_flat.py's tolerances, each schedule alone and all together, capacity against exact count, writes that stay
inside the outputs and the workspace, the unmarked call bit-equal to the call composed as before, and a recorded call replayed
on another matrix inside the capacities.

The graph: 300 nodes; row 1 holds 600 entries from entry 5 on (columns repeat: a hub row that crosses the chunk ends at 256
and 512), row 10 has only negative values (dead under the GAT mask), row 20 is empty, the others are short; a fifth of the
values are negative (masked)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _layer_grad_ref as LG
import _spmm_flat_ref as F

pytestmark = pytest.mark.gpu
N, M_FEA, ALPHA = 300, 20, 0.2
HUB, DEAD, EMPTY = 1, 10, 20
SENTINEL = -77.0
GRAD_TOL = dict(grad_input=1e-5, grad_weights=1e-5, grad_attention=1e-7)       # test_gpu_layer_flat.py's, for the same gradients
TDT = {"f16": torch.float16, "f32": torch.float32}


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def graph(dt, seed=0):
    deg = list(np.random.default_rng(5 + seed).poisson(5.0, N) + 1)
    deg[0], deg[HUB], deg[EMPTY] = 5, 600, 0
    rp, ci, va = F.build(deg, N, dt, seed=seed)
    neg = np.random.default_rng(9 + seed).random(len(va)) < 0.2
    va = np.where(neg, -np.abs(va), np.abs(va))
    va[rp[DEAD]:rp[DEAD + 1]] = -np.abs(va[rp[DEAD]:rp[DEAD + 1]])
    va[rp[HUB]:rp[HUB] + 300] = np.abs(va[rp[HUB]:rp[HUB] + 300])
    return rp, ci, va


def csr_of(g, dt, capacity=None, n_cols=N, **facts):
    """col / val hold `capacity` entries; those behind the end are a column far outside and a NaN, never to be read"""
    from sgracex1_amd import ops
    rp, ci, va = g
    cap = len(ci) if capacity is None else capacity
    col = torch.full((cap,), 1 << 30, dtype=torch.int32, device="cuda")
    val = torch.full((cap,), float("nan"), dtype=TDT[dt] if isinstance(dt, str) else dt, device="cuda")
    col[:len(ci)] = torch.as_tensor(ci)
    val[:len(ci)] = torch.as_tensor(va).to(val.dtype)
    A = ops.Csr(torch.as_tensor(rp, dtype=torch.int32, device="cuda"), col, val, n_cols)
    return A.with_facts(**facts) if facts else A


@functools.lru_cache(maxsize=None)
def operands(P, seed=0):
    """X fp32 [N, M_FEA] (60 % zeros, on the fp16 grid), W [M_FEA, P], the attention vector [2 P], G [N, P]"""
    g = torch.Generator().manual_seed(100 + P + seed)
    X = ((torch.rand((N, M_FEA), generator=g) - 0.3) * (torch.rand((N, M_FEA), generator=g) < 0.4)).half().float()
    W = ((torch.rand((M_FEA, P), generator=g) * 2 - 1) / M_FEA ** 0.5).half().float()
    att = (torch.randn(2 * P, generator=g) / P ** 0.5).half().float()
    G = torch.randn((N, P), generator=g)
    return X.cuda(), W.cuda(), att.cuda(), G.cuda()


def feature_pair(X, flat, extra=0):
    """(CSR of X, CSR of X^T) in fp32 at `extra` entries of capacity above their count, flat-marked or not"""
    sp = X.cpu().to_sparse_csr()
    xc = (sp.crow_indices().numpy().astype(np.int32), sp.col_indices().numpy().astype(np.int32), sp.values().numpy())
    st = X.cpu().t().contiguous().to_sparse_csr()
    xt = (st.crow_indices().numpy().astype(np.int32), st.col_indices().numpy().astype(np.int32), st.values().numpy())
    facts = dict(flat=True) if flat else {}
    return (csr_of(xc, "f32", len(xc[1]) + extra, n_cols=M_FEA, **facts), csr_of(xt, "f32", len(xt[1]) + extra, n_cols=N, **facts))


def forward_state(A, X, W, att, lean):
    """what the forward keeps for the backward: (E, S) or the statistics, and the dead rows -- from the layer's own forward"""
    from sgracex1_amd import ops
    plain = ops.Csr(A.rowptr, A.col, A.val, A.n_cols)
    fea, Wt = X.to(A.val.dtype).contiguous(), W.t().to(A.val.dtype).contiguous()
    kw = dict(gat_attention=att.to(A.val.dtype), alpha=ALPHA, fill_dead_rows=True)
    out, E, S = ops.layer_forward(plain, fea, Wt, want_edge_outputs=True, **kw)
    dead = LG.dead_rows_of(A.rowptr, A.val.float())
    assert bool(dead[DEAD]) and bool(dead[EMPTY]) and not bool(dead[HUB])
    if not lean:
        return dict(E=E, S=S, dead=dead), (E, S, dead)
    _, stats = ops.layer_forward(plain, fea, Wt, want_row_stats=True, **kw)
    return dict(stats=stats, dead_weight=1.0 / N, dead=dead), (E, S, dead)


# ---- the named stage calls, composed as sgx_layer_backward composes them ----------------------------------------------------

def composed(A, X, W, G, gat, gemm, state, flat_adj, flat_fea, flat_xt, want_grad_input=True):
    from sgracex1_amd import _lib, ops
    lib, stream = _lib.lib, torch.cuda.current_stream().cuda_stream
    n, (M, P) = A.n_rows, W.shape
    ldwh = ops.table_pitch(P, 4)
    sched = lambda f: "flat" if f else None
    plain = lambda c: ops.Csr(c.rowptr, c.col, c.val, c.n_cols)             # the same arrays without the fact
    out = {}
    if gat:
        Wh = torch.full((n, ldwh), float("nan"), device="cuda")
        if gemm == 1:
            ops.xw_dense(X.float().contiguous(), ops.transpose(W), ldh=ldwh, out=Wh[:, :P])
        elif flat_fea:
            ops.spmm(plain(X[0]), W, n_feat=P, out=Wh[:, :P], schedule="flat")
        else:
            ops.xw_sparse(plain(X[0]), W, out=Wh[:, :P])
        dead, drs = state.get("dead"), None
        if dead is not None:                                                  # G[r] . (colsum(Wh) * (1 / N)) through sgx_xw_dense
            inv_n = float(np.float32(1.0) / np.float32(n))
            mean = (ops.col_sums(Wh[:, :P]) * inv_n).contiguous()
            tmp = torch.empty((n, 4), device="cuda")
            ops.check(lib.sgx_xw_dense(_lib.SGX_F32, _lib.SGX_ACC_F32, 1, n, P, 1, G.data_ptr(), G.stride(0), mean.data_ptr(), P,
                                       tmp.data_ptr(), 4, stream), "sgx_xw_dense")
            drs = tmp[:, 0].contiguous()
        sg = torch.full((A.nnz + 1,), float("nan"), device="cuda")
        g1 = torch.empty(n, device="cuda")
        code = ops.dtype_code(A.val.dtype)
        dptr = lambda t: None if t is None else t.data_ptr()
        if "stats" in state:
            S = torch.full((A.nnz + 1,), float("nan"), device="cuda")
            st = state["stats"].struct()
            ops.check(lib.sgx_gat_backward_edges_stats(code, n, n, P, 1, ALPHA, A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(),
                                                       ctypes.byref(st), state["dead_weight"], G.data_ptr(), G.stride(0), Wh.data_ptr(),
                                                       ldwh, dptr(dead), dptr(drs), sg.data_ptr(), g1.data_ptr(), S.data_ptr(), stream),
                      "sgx_gat_backward_edges_stats")
        else:
            S = state["S"]
            ops.check(lib.sgx_gat_backward_edges(code, n, n, P, ALPHA, A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(),
                                                 state["E"].data_ptr(), S.data_ptr(), G.data_ptr(), G.stride(0), Wh.data_ptr(), ldwh,
                                                 dptr(dead), dptr(drs), sg.data_ptr(), g1.data_ptr(), stream), "sgx_gat_backward_edges")
        out["grad_attention"] = ops.gat_attention_grad(plain(A), sg, g1, Wh[:, :P], schedule=sched(flat_adj))
        Pm = ops.Csr(A.rowptr, A.col, S[:A.nnz] if S.numel() > A.nnz else S, A.n_cols)
    else:
        Pm = ops.Csr(A.rowptr, A.col, A.val.float(), A.n_cols)
    pg = ops.spmm(Pm, G, schedule="flat") if flat_adj else ops.spmm(Pm, G, use_plan=False)
    if gat and state.get("dead") is not None:
        inv_n = float(np.float32(1.0) / np.float32(n))
        pg = torch.where(state["dead"].unsqueeze(1), (ops.col_sums(G) * inv_n).unsqueeze(0), pg)
    if want_grad_input:
        out["grad_input"] = ops.xw_dense(pg, W.contiguous(), ldh=ops.table_pitch(M, 4))[:, :M]
    if gemm == 1:
        out["grad_weights"] = ops.xt_g(X, pg)
    else:
        out["grad_weights"] = ops.spmm(plain(X[1]), pg, schedule="flat") if flat_xt else ops.spmm(plain(X[1]), pg, use_plan=False)
    return out


def one_call(A, X, W, G, gat, gemm, state, schedule=None, want_grad_input=True):
    from sgracex1_amd import ops
    gi, gw, ga = ops.layer_backward(A, X, W, G, gat=bool(gat), gemm_mode=gemm, alpha=ALPHA, schedule=schedule,
                                    want_grad_input=want_grad_input, **state)
    out = dict(grad_weights=gw)
    if gi is not None:
        out["grad_input"] = gi
    if gat:
        out["grad_attention"] = ga
    return out


def assert_same_bits(got, want, what):
    assert got.keys() == want.keys(), what
    for k in got:
        assert torch.equal(bits(got[k]), bits(want[k])), (what, k, float((got[k] - want[k]).abs().max()))


def restated(g, dt, X, W, G, gat, ES):
    rp, ci, va = g
    val = torch.as_tensor(va).to(TDT[dt])
    kw = dict(E=ES[0][:len(ci)].cpu(), S=ES[1][:len(ci)].cpu(), dead=ES[2].cpu()) if gat else {}    # (E, S may hold a capacity)
    # (the edge-list form: the hub row repeats columns, and mask and slope are facts of an entry, not of a matrix element)
    return LG.edges(torch.as_tensor(rp), torch.as_tensor(ci), val, X.cpu(), W.cpu(), G.cpu(), gat=bool(gat), alpha=ALPHA, **kw)


def check_float64(got, ref, what):
    shaped = {k: (v.unsqueeze(1) if k == "grad_attention" else v) for k, v in got.items()}
    figures = LG.check({k: v.cpu() for k, v in shaped.items()}, ref[0], ref[1], GRAD_TOL, what)
    print("layer_backward_flat", what, {k: f"{v:.2e}" for k, v in figures.items()})


# ---- 1. the bit rule and float64, every axis ----------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [3, 64])
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("gemm", [1, 0], ids=["dense", "csr"])
@pytest.mark.parametrize("mode", ["gcn", "gat_es", "gat_stats"])
def test_bit_rule_and_float64(mode, gemm, dt, P):
    from sgracex1_amd import _lib
    gat, lean = int(mode != "gcn"), mode == "gat_stats"
    g = graph(dt)
    X, W, att, G = operands(P)
    A = csr_of(g, dt, flat=True)
    Xop = feature_pair(X, flat=True) if gemm == 0 else (X.half() if dt == "f16" else X)
    state, ES = forward_state(A, X, W, att, lean) if gat else ({}, None)
    assert route_of(A, Xop, W, G, gat, gemm, state) == (1 if gemm == 1 else (7 if gat else 5))
    got = one_call(A, Xop, W, G, gat, gemm, state)
    want = composed(A, Xop, W, G, gat, gemm, state, True, gemm == 0, gemm == 0)
    assert_same_bits(got, want, (mode, gemm, dt, P))
    assert A._plan is None and (gemm == 1 or (Xop[0]._plan is None and Xop[1]._plan is None))     # no plan was built on the way
    again = one_call(A, Xop, W, G, gat, gemm, state)
    assert_same_bits(again, got, "two runs")
    check_float64(got, restated(g, dt, X, W, G, gat, ES), (mode, gemm, dt, P))
    # grad_input left out: the other outputs keep their bits
    partial = one_call(A, Xop, W, G, gat, gemm, state, want_grad_input=False)
    assert "grad_input" not in partial
    assert_same_bits(partial, {k: v for k, v in got.items() if k != "grad_input"}, "no grad_input")


# ---- 2. each schedule alone and all together, the route asserted ----------------------------------------------------------------

def route_of(A, X, W, G, gat, gemm, state, schedule=None):
    """sgx_layer_backward_schedule on the descriptor ops.layer_backward itself builds for these operands"""
    from sgracex1_amd import ops
    return ops.layer_backward_schedule(A, X, W, G, gat=bool(gat), gemm_mode=gemm, alpha=ALPHA, schedule=schedule, **state)


@pytest.mark.parametrize("route", range(8))
@pytest.mark.parametrize("gat", [0, 1], ids=["gcn", "gat"])
def test_each_schedule_alone_and_together(gat, route):
    P = 64
    g = graph("f32")
    X, W, att, G = operands(P)
    fa, ff, fx = bool(route & 1), bool(route & 2), bool(route & 4)
    A = csr_of(g, "f32", **(dict(flat=True) if fa else {}))
    Xc, _ = feature_pair(X, flat=ff)
    _, Xt = feature_pair(X, flat=fx)
    state, ES = forward_state(A, X, W, att, lean=True) if gat else ({}, None)
    assert route_of(A, (Xc, Xt), W, G, gat, 0, state) == (route if gat else route & 5)
    assert route_of(A, (Xc, Xt), W, G, gat, 0, state, "flat") == (7 if gat else 5) and route_of(A, (Xc, Xt), W, G, gat, 0, state, "rows") == 0
    got = one_call(A, (Xc, Xt), W, G, gat, 0, state)
    assert_same_bits(got, composed(A, (Xc, Xt), W, G, gat, 0, state, fa, ff and gat, fx), ("route", route, gat))
    check_float64(got, restated(g, "f32", X, W, G, gat, ES), ("route", route, gat))
    # the keyword overrides the facts both ways
    everything = one_call(A, (Xc, Xt), W, G, gat, 0, state, schedule="flat")
    assert_same_bits(everything, composed(A, (Xc, Xt), W, G, gat, 0, state, True, bool(gat), True), ("keyword flat", route))
    by_rows = one_call(A, (Xc, Xt), W, G, gat, 0, state, schedule="rows")
    assert_same_bits(by_rows, composed(A, (Xc, Xt), W, G, gat, 0, state, False, False, False), ("keyword rows", route))


# ---- 3. the unmarked call is unchanged ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gemm", [1, 0], ids=["dense", "csr"])
@pytest.mark.parametrize("mode", ["gcn", "gat_es", "gat_stats"])
def test_unmarked_call_equals_the_call_composed_as_before(mode, gemm):
    gat, lean = int(mode != "gcn"), mode == "gat_stats"
    for dt in ("f16", "f32"):
        g = graph(dt)
        X, W, att, G = operands(64)
        A = csr_of(g, dt)
        Xop = feature_pair(X, flat=False) if gemm == 0 else (X.half() if dt == "f16" else X)
        state, _ = forward_state(A, X, W, att, lean) if gat else ({}, None)
        assert route_of(A, Xop, W, G, gat, gemm, state) == 0
        got = one_call(A, Xop, W, G, gat, gemm, state)
        assert_same_bits(got, composed(A, Xop, W, G, gat, gemm, state, False, False, False), ("unmarked", mode, gemm, dt))


# ---- 4. capacity against exact count; writes stay inside ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["gcn", "gat_stats"])
def test_capacity_gives_the_exact_count_bits(mode):
    from sgracex1_amd import _lib
    gat = int(mode != "gcn")
    T = _lib.lib.sgx_spmm_flat_chunk()
    g = graph("f32")
    X, W, att, G = operands(64)
    exact_A = csr_of(g, "f32", flat=True)
    state, _ = forward_state(exact_A, X, W, att, lean=True) if gat else ({}, None)
    want = one_call(exact_A, feature_pair(X, flat=True), W, G, gat, 0, state)
    for extra in (1, 3 * T):
        A = csr_of(g, "f32", len(g[1]) + extra, flat=True)
        assert A.nnz == len(g[1]) + extra
        got = one_call(A, feature_pair(X, flat=True, extra=extra), W, G, gat, 0, state)
        assert_same_bits(got, want, ("capacity", mode, extra))


@pytest.mark.parametrize("gemm", [1, 0], ids=["dense", "csr"])
def test_writes_stay_inside_outputs_and_workspace(gemm):
    """the descriptor built by hand: outputs and workspace prefilled with NaN between sentinels"""
    from sgracex1_amd import _lib, ops
    P, guard = 64, 64
    g = graph("f32")
    X, W, att, G = operands(P)
    A = csr_of(g, "f32", len(g[1]) + 100, flat=True)
    Xop = feature_pair(X, flat=True, extra=50) if gemm == 0 else X
    state, _ = forward_state(A, X, W, att, lean=True)
    want = one_call(A, Xop, W, G, 1, gemm, state)
    d = _lib.LayerGradDesc()
    d.gat_mode, d.gemm_mode, d.N_adj, d.M_adj, d.M_fea, d.P_w = 1, gemm, N, N, M_FEA, P
    d.dtype_adj, d.dtype_x, d.gat_heads, d.alpha, d.nnz_adj = _lib.SGX_F32, _lib.SGX_F32, 1, ALPHA, A.nnz
    d.rowPtr_adj, d.columnIndex_adj, d.values_adj = A.rowptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr()
    d.schedule_adj = _lib.SGX_SCHEDULE_FLAT
    if gemm == 1:
        d.X, d.ldx = X.data_ptr(), X.stride(0)
    else:
        Xc, Xt = Xop
        d.rowPtr_fea, d.columnIndex_fea, d.values_fea = Xc.rowptr.data_ptr(), Xc.col.data_ptr(), Xc.val.data_ptr()
        d.rowPtr_xt, d.columnIndex_xt, d.values_xt = Xt.rowptr.data_ptr(), Xt.col.data_ptr(), Xt.val.data_ptr()
        d.schedule_fea = d.schedule_xt = _lib.SGX_SCHEDULE_FLAT
        d.nnz_fea, d.nnz_xt = Xc.nnz, Xt.nnz
    st = state["stats"].struct()
    d.stats, d.dead_weight, d.dead = ctypes.pointer(st), state["dead_weight"], state["dead"].data_ptr()
    d.W, d.G, d.ldg = W.data_ptr(), G.data_ptr(), G.stride(0)
    ld_gi = ops.table_pitch(M_FEA, 4)
    sizes = dict(grad_weights=M_FEA * P, grad_attention=2 * P, grad_input=N * ld_gi)
    bufs = {}
    for name, size in sizes.items():
        b = torch.full((size + 2 * guard,), SENTINEL, device="cuda")
        b[guard:guard + size] = float("nan")
        bufs[name] = b
        setattr(d, name, b[guard:].data_ptr())
    d.ld_gi = ld_gi
    assert _lib.lib.sgx_layer_backward_schedule(ctypes.byref(d)) == (1 if gemm == 1 else 7)
    need = _lib.lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d))
    assert need > 0 and need % 256 == 0
    ws = torch.full((need // 4 + 2 * guard,), SENTINEL, device="cuda")
    ws[guard:guard + need // 4] = float("nan")
    assert ws[guard:].data_ptr() % 256 == 0
    d.workspace, d.workspace_bytes = ws[guard:].data_ptr(), need
    ops.check(_lib.lib.sgx_layer_backward(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "sgx_layer_backward")
    for name, b in list(bufs.items()) + [("workspace", ws)]:
        size = sizes.get(name, need // 4)
        assert (b[:guard] == SENTINEL).all() and (b[guard + size:] == SENTINEL).all(), name
    got = dict(grad_weights=bufs["grad_weights"][guard:guard + M_FEA * P].view(M_FEA, P),
               grad_attention=bufs["grad_attention"][guard:guard + 2 * P],
               grad_input=bufs["grad_input"][guard:guard + N * ld_gi].view(N, ld_gi)[:, :M_FEA])
    assert_same_bits(got, want, ("by hand", gemm))
    assert not bufs["grad_input"][guard:guard + N * ld_gi].view(N, ld_gi)[:, M_FEA:].any()          # pad columns zeroed


# ---- 5. recorded and replayed on another matrix inside the capacities --------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["gcn", "gat_stats"])
def test_recorded_call_replays_on_another_matrix(mode):
    from sgracex1_amd import ops
    gat = int(mode != "gcn")
    first, second = graph("f32"), graph("f32", seed=1)
    cap = max(len(first[1]), len(second[1])) + 300
    X, W, att, G = operands(64)
    A = csr_of(first, "f32", cap, flat=True)
    Xop = feature_pair(X, flat=True, extra=40)
    state1, _ = forward_state(A, X, W, att, lean=True) if gat else ({}, None)
    eager_first = one_call(A, Xop, W, G, gat, 0, state1)                         # sizes the workspace outside the recording
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.graph(graph_):
            out = one_call(A, Xop, W, G, gat, 0, state1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert A._plan is None and Xop[0]._plan is None and Xop[1]._plan is None
    graph_.replay()
    assert_same_bits(out, eager_first, "replay on the recorded matrix")
    B = csr_of(second, "f32", cap, flat=True)
    state2, ES2 = forward_state(B, X, W, att, lean=True) if gat else ({}, None)
    want = one_call(B, Xop, W, G, gat, 0, state2)
    A.rowptr.copy_(B.rowptr), A.col.copy_(B.col), A.val.copy_(B.val)
    if gat:
        for a, b in zip(state1["stats"].tensors(), state2["stats"].tensors()):
            a.copy_(b)
        state1["dead"].copy_(state2["dead"])
    graph_.replay()
    assert_same_bits(out, want, "replay on the second matrix")
    check_float64(out, restated(second, "f32", X, W, G, gat, ES2), ("replayed", mode))


# ---- 6. ops.feature_csr32 off the loader path -------------------------------------------------------------------------------

def test_feature_csr32_hands_on_the_flat_fact_of_a_cached_feature_csr():
    """a feature tensor whose forward CSR was marked by hand: the fp32 pair built for the backward is flat-marked, wants no
    plan, holds X and X^T, and the call takes all three entry-split routes; without the mark the pair is unmarked"""
    from sgracex1_amd import ops
    X, W, _, G = operands(64)
    A = csr_of(graph("f32"), "f32", flat=True)
    x = X.clone()
    ops.attach(x, ("fea_csr", torch.float16), ops.Csr.from_dense(x, torch.float16).with_facts(flat=True))
    Xc, Xt = ops.feature_csr32(x)
    assert Xc._flat and Xt._flat and not Xc.wants_plan and not Xt.wants_plan and Xc._plan is None and Xt._plan is None
    assert Xc.val.dtype == torch.float32 and (Xc.n_rows, Xc.n_cols, Xt.n_rows, Xt.n_cols) == (N, M_FEA, M_FEA, N)
    assert route_of(A, x, W, G, 0, 0, {}) == 5
    ref = feature_pair(X, flat=True)
    assert_same_bits(one_call(A, x, W, G, 0, 0, {}), one_call(A, ref, W, G, 0, 0, {}), "feature_csr32")
    plain = X.clone()
    Pc, Pt = ops.feature_csr32(plain)
    assert not Pc._flat and not Pt._flat and route_of(A, plain, W, G, 0, 0, {}) == 1
