"""The quantised layer's two store epilogues (sgx_epilogue, csrc/sgx_internal.h: the re-quantisation of H = X.W on stage 1's
stores, deq_o after the ReLU on stage 2's) on every kernel path that carries one.  tests/test_gpu_quant.py runs the layer
at one family of small shapes, where the dispatcher picks the same few store sites each time; here each case builds the
shape that selects one path, asserts the plan / shape fact that selects it, and makes two checks:

 (a) fused == unfused, torch.equal.  The chain is built from public ops whose stores carry no epilogue: fake_quantize on
     the operands, xw_sparse / xw_dense (the layer's H pitch) / xw_dense_i8(.., 0, 0), requantize_, spmm / gat_aggregate,
     one torch fp32 multiply by deq_o -- on the same Csr objects and plans, under the same tuning overrides.  The same
     kernel forms the same fp32 sums and the epilogue is the same fp32 operation once per element, so the bits are equal:
     a store site that drops its epilogue, applies it twice (task and finalize) or applies it to a fill row differs.
 (b) the chain's H against the exact integer sums of tests/_quant_ref.py, bit for bit (each case asserts the 2^24
     condition from its own operands), and the fused D inside the derived stage-2 bound (GAT: tests/_gat_ref.py's).

No case needed (a) weakened to the bound: no path's summation order differs between the layer and the chain.
Stage-1 cases run the layer on an identity adjacency handed over as already quantised (D = relu-less H deq_o), on large
matrices against the reference on a sample of rows (the empty rows and the ends among them).  There are no tolerances here
but the bounds named above.  Not reached: the several-heads one-pass kernel's store (one head here) and, at F = 24, the
one walk of gat_fused.hip (it runs at F = 64)."""
import numpy as np
import pytest
import torch

import _quant_ref as Q
from test_gpu_gat_paths import FORMS, Case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _csr(triple, n_cols):
    from sgracex1_amd import ops
    rp, col, val = triple
    return ops.Csr(_dev(rp, torch.int32), _dev(col, torch.int32), _dev(val), n_cols)


def _eye(n):
    from sgracex1_amd import ops
    return ops.Csr(torch.arange(n + 1, dtype=torch.int32, device=DEV), torch.arange(n, dtype=torch.int32, device=DEV),
                   torch.ones(n, device=DEV), n)


def _constants(bits, deq=None):
    from sgracex1_amd import quant
    return quant.constants(bits) if deq is None else quant.constants(bits, deq_o=deq)


def chain_H(X, Wt, c):
    """Stage 1 unfused: quantised operands, the plain product into a buffer of the layer's H pitch, requantize_."""
    from sgracex1_amd import ops
    b, (P, _M) = c.w_qbits, Wt.shape
    ldh = ops.table_pitch(P, 4)
    Wq = ops.fake_quantize(Wt, 1, b, c.w_s, c.w_z)
    assert Wq.stride(0) == _M and Wq.data_ptr() % 16 == 0             # the pitch and alignment of the layer's own copy
    if isinstance(X, ops.Csr):
        Xq = ops.Csr(X.rowptr, X.col, ops.fake_quantize(X.val, 0, b, c.f_s, c.f_z), X.n_cols, X.plan if X.wants_plan else None)
        W = ops.transpose(Wq, ldo=ldh)                                   # [M, ldh], as the layer lays W out
        buf = torch.zeros((X.n_rows, ldh), device=DEV)
        H = ops.xw_sparse(Xq, W[:, :P], out=buf[:, :P])
    else:
        H = ops.xw_dense(ops.fake_quantize(X, 0, b, c.f_s, c.f_z), Wq, ldh=ldh)
    assert H.stride(0) == ldh
    return ops.requantize_(H, c.scale_fea, c.internal_quantization)


def _sample(n, must=(), seed=0):
    if n <= 6000:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([rng.choice(n, 1024, replace=False), np.asarray(must, np.int64), [0, n - 1]]))


def _stage1(X, X_host, W, c, clip_terms, empty=None):
    """(a) and (b) for one X.W path: the layer on an identity adjacency.  Returns the fused D."""
    from sgracex1_amd import ops
    n = X.n_rows if isinstance(X, ops.Csr) else X.shape[0]
    Wt = _dev(W.T)
    eye = _eye(n)
    fused = ops.layer_forward(eye, X, Wt, relu=False, quant=c, adj_quantized=True)
    H = chain_H(X, Wt, c)
    chain = ops.spmm(eye, H, relu=False) * Q.deq32(c)
    assert torch.equal(fused, chain), f"{int((fused != chain).sum())} elements differ from the unfused chain"
    rows = _sample(n, must=() if empty is None else empty[:8], seed=n)
    Href, mag, facts = Q.stage1(X_host, W, c, rows=rows)
    t_rows = torch.as_tensor(rows, device=DEV)
    Q.check_H(H[t_rows].cpu().numpy(), Href, mag)
    k = len(rows)
    D, bound = Q.stage2_gcn((np.arange(k + 1), np.arange(k)), np.ones(k, np.float32), Href, c, relu=False)
    Q.check_D(fused[t_rows].cpu().numpy(), D, bound)
    Q.assert_edges(dict(H=Href, facts=facts), c, clip_terms=clip_terms)
    if empty is not None:
        assert len(empty) > 0 and not fused[torch.as_tensor(empty, device=DEV)].any()        # the requantised 0, scaled
    assert fused.abs().max() > 0
    return fused


# ---- stage 1, sparse X ------------------------------------------------------------------------------------------------

_store = {}


def _sparse_x(key, build):
    """One CSR X per path, shared by its bit widths (the helper's X does not depend on them), left unchanged."""
    if key not in _store:
        n, m, degs, hot_every = build()
        seed = sum(map(ord, repr(key)))                  # from the key alone: the same X whichever tests ran before
        host = Q.features(n, m, None, seed, degs=degs, hot_every=hot_every)
        _store[key] = (host, _csr(host, m), np.nonzero(degs == 0)[0], int(np.median(degs[::hot_every])))
    return _store[key]


def _lds_degs(m):
    def build():
        rng = np.random.default_rng(m)
        n = 8192
        degs = rng.integers(129, 134, n)            # ~131 entries per row: just over 2^20 in all, far below the plan's cut
        degs[5::211] = 0
        return n, m, degs, 7
    return build


# (M, P): 4 lanes x 4 slices; one slice; a ragged last slice with element stores
@pytest.mark.parametrize("M,P", [(1433, 64), (300, 16), (1000, 41)])
@pytest.mark.parametrize("bits", [8, 4, 2, 1])
def test_stage1_sparse_lds_form(M, P, bits):
    from sgracex1_amd import _lib, ops
    host, X, empty, hot = _sparse_x(("lds", M), _lds_degs(M))
    # selects xw_sparse_lds.hip: 2^20 entries and more, 4096 rows and more, a plan that cuts no row and carries win_order
    assert X.nnz >= 1 << 20 and X.n_rows >= 4096 and X.plan.long_rows == 0 and X.plan.export("win_order").numel() > 0
    c = _constants(bits)
    W = Q.weights(M, P, c, M + P)
    fused = _stage1(X, host, W, c, hot, empty)
    with _lib.tuning(SGX_XW_SPARSE_NO_LDS="1"):             # the gather kernel on the same matrix: the same bits
        gather = ops.layer_forward(_eye(X.n_rows), X, _dev(W.T), relu=False, quant=c, adj_quantized=True)
    assert torch.equal(fused, gather)


def _cut_degs():
    rng = np.random.default_rng(64)
    n, m = 3000, 300
    degs = rng.integers(0, 20, n)
    degs[::7] = 24                                  # hot rows: enough terms to clip at every bit width
    degs[[14, 497, 1505]] = [65, 200, m]            # long hot rows (multiples of 7) ...
    degs[[11, 501]] = [65, 130]                     # ... and long rows of ordinary values
    return n, m, degs, 7


@pytest.mark.parametrize("bits", [8, 4, 2, 1])
def test_stage1_sparse_gather_kernel_with_cut_rows(bits):
    """Rows of 65, 200 and M entries among short ones: the tasks' partial rows must stay plain sums, the finalize kernel
    (spmm_split_finalize_kernel) applies the epilogue once."""
    host, X, empty, hot = _sparse_x("cut", _cut_degs)
    # under 2^20 entries the plan cuts rows above 64 entries; no LDS form there
    assert 8192 <= X.nnz < 1 << 20 and X.plan.long_threshold == 64 and X.plan.long_rows == 5
    c = _constants(bits)
    _stage1(X, host, Q.weights(300, 24, c, 5), c, hot, empty)


def _short_degs():
    rng = np.random.default_rng(2)
    n, m = 6000, 200
    degs = rng.integers(0, 5, n)
    degs[::50] = 40
    return n, m, degs, 50


@pytest.mark.parametrize("bits", [8, 2])
def test_stage1_sparse_two_chunks_per_lane(bits):
    host, X, empty, hot = _sparse_x("cpl2", _short_degs)
    P = 24
    # choose_cpl: a plan whose mean degree is below kShortRowDegree = 5 and rows of two 16-byte chunks and more: CPL = 2
    assert X.wants_plan and X.nnz / X.n_rows < 5.0 and P > 4 and X.plan.long_rows == 0
    c = _constants(bits)
    _stage1(X, host, Q.weights(200, P, c, 9), c, hot, empty)


# ---- stage 1, dense X -------------------------------------------------------------------------------------------------

# name: (n, M, P); the rule of sgx_xw_dense_ep that selects the form is asserted in the test
DENSE = {"stationary": (8192 + 11, 16, 16), "wlds": (32768 + 5, 64, 129), "tile": (1000, 130, 47), "tall": (32768 + 37, 300, 128)}


@pytest.mark.parametrize("form", list(DENSE))
@pytest.mark.parametrize("bits", [8, 2])
def test_stage1_dense_fp32_forms(form, bits):
    from sgracex1_amd import _lib, ops
    n, M, P = DENSE[form]
    cols = ops.table_pitch(P, 4)
    # sgx_xw_dense_wlds_f32: W^T rows are read 16 bytes at a time, so their pitch (M floats, in the layer's quantised copy
    # and in the chain's alike) must be a multiple of 4 and the base 16-byte aligned (the layer's 256-byte aligned
    # workspace; chain_H asserts its own) -- M = 33 would fall through to the stationary kernel
    wlds = 32 < M <= 128 and M % 4 == 0 and 64 < cols <= 1024 and n >= 32768
    stationary = M <= 128 and n >= 8192                                    # try_stationary_f32 (after the LDS form)
    assert {"wlds": wlds, "stationary": stationary and not wlds, "tile": not wlds and not stationary and n < 32768,
            "tall": not wlds and not stationary and n >= 32768 and (cols + 15) // 16 >= 8}[form]
    c = _constants(bits)
    if ("dense", form) not in _store:
        host = Q.features(n, M, c, n, dense=True)
        _store[("dense", form)] = (host, _dev(host))
    host, X = _store[("dense", form)]
    W = Q.weights(M, P, c, M * P)
    fused = _stage1(X, host, W, c, M)
    with _lib.tuning(SGX_XW_NO_STATIONARY_F32="1", SGX_XW_NO_WLDS="1"):       # the tile kernel: the same bits
        tile = ops.layer_forward(_eye(n), X, _dev(W.T), relu=False, quant=c, adj_quantized=True)
        assert torch.equal(tile, ops.spmm(_eye(n), chain_H(X, _dev(W.T), c), relu=False) * Q.deq32(c))
    assert torch.equal(fused, tile)


@pytest.mark.parametrize("n,M,P", [(777, 130, 47), (40, 7, 3)])
@pytest.mark.parametrize("bits", [8, 2])
def test_stage1_int8_epilogue(n, M, P, bits):
    """sgx_xw_dense_i8 with its epilogue == requantize_ of the call without == the exact reference (ragged K, P, rows)."""
    from sgracex1_amd import ops
    c = _constants(bits)
    X, W = Q.features(n, M, c, n + bits, dense=True), Q.weights(M, P, c, M + bits)
    Xc, _xb = ops.quantize_codes_i8(_dev(X), 0, bits, c.f_s, c.f_z)
    Wc, _wb = ops.quantize_codes_i8(_dev(W.T), 1, bits, c.w_s, c.w_z)
    plain = ops.xw_dense_i8(Xc, Wc, M, bits, 0, 0)
    fused = ops.xw_dense_i8(Xc, Wc, M, bits, c.scale_fea, c.internal_quantization)
    assert torch.equal(fused, ops.requantize_(plain.clone(), c.scale_fea, c.internal_quantization))
    Href, mag, facts = Q.stage1(X, W, c)
    Q.check_H(fused.cpu().numpy(), Href, mag)
    Q.assert_edges(dict(H=Href, facts=facts), c, clip_terms=M)
    assert plain.abs().max() > fused.abs().max() > 0


# ---- stage 2, GCN aggregate -------------------------------------------------------------------------------------------

class _Graph:
    """One adjacency on the device with its plans; plan() is the GAT path tests' own helper."""
    plan = Case.plan

    def __init__(self, degs, seed):
        self.degs, self.n = degs, len(degs)
        c8 = _constants(8)
        rp, col, _v = Q.adjacency(degs, self.n, c8, seed)
        self.rp, self.colh = rp, col
        self.rowptr, self.col = _dev(rp, torch.int32), _dev(col, torch.int32)
        self.seed = seed
        self._plans, self._gcn_plans, self._vals = {}, {}, {}

    def values(self, c, dead_rows=()):
        """The unquantised values for these constants (the adjacency range moves with the bit width)."""
        if c.w_qbits not in self._vals:
            self._vals[c.w_qbits] = Q.adjacency(self.degs, self.n, c, self.seed, dead_rows=dead_rows)[2]
        return self._vals[c.w_qbits]

    def gcn_plan(self, kind):
        from sgracex1_amd import _lib, ops
        if kind not in self._gcn_plans:
            with _lib.tuning(SGX_PLAN_REORDER_BELOW="2" if kind == "ordered" else "0"):
                self._gcn_plans[kind] = ops.Plan(self.rowptr)
        return self._gcn_plans[kind]


def _gcn_degs():
    rng = np.random.default_rng(20)
    n = 20_000
    degs = np.where(np.arange(n) % 2 == 0, rng.integers(0, 9, n), rng.integers(9, 52, n))
    degs[[3, 100, 101]] = [3000, 65, 200]            # a hub row and two more above the cut of 64
    return degs


@pytest.fixture(scope="module")
def gcn_graph():
    return _Graph(_gcn_degs(), 20)


@pytest.mark.parametrize("kind,P,deq", [("natural", 24, None), ("ordered", 24, None), ("natural", 41, None), ("ordered", 47, None),
                                        ("natural", 4, None), ("ordered", 4, None), ("natural", 24, -0.37), ("ordered", 24, -0.37)])
@pytest.mark.parametrize("bits", [8, 2])
def test_stage2_gcn_aggregate(gcn_graph, kind, P, deq, bits):
    """natural order / degree order (with its one-step tail at P = 24), a hub row through tasks and the finalize kernel,
    D rows that are only element-aligned (P = 41, 47), one lane per row (P = 4), and a negative deq_o: ReLU, then scale."""
    from sgracex1_amd import _lib, ops
    g, M = gcn_graph, 16
    c = _constants(bits, deq)
    plan = g.gcn_plan(kind)
    nnz = int(g.rp[-1])
    # under 2^20 entries: rows above 64 entries are cut into tasks (split path + spmm_split_finalize_kernel)
    assert nnz < 1 << 20 and plan.reordered == (kind == "ordered") and plan.long_rows >= 3 and plan.long_threshold == 64
    assert nnz / g.n >= 5.0                                               # CPL = 1 (choose_cpl)
    if P in (41, 47):
        assert (P * 4) % 16 != 0                                          # rows of D start off 16-byte boundaries
    tail = kind == "ordered" and P == 24
    if tail:
        # launch_one_impl: a degree order whose last 4096 rows and more take one step (<= 8 entries), P within one pass
        # of LPR = 8 lanes x 4 columns
        assert 16 < P <= 32
        # ... read from the plan's own order: rows by steps of 8 entries, longest first; n_multi = the rows of two steps
        # and more, and the tail behind them is what spmm_short_tail_kernel takes 64 rows to a wavefront
        order = plan.export("row_order").cpu().numpy()
        steps = (g.degs[order] + 7) // 8
        assert (np.diff(steps) <= 0).all() and steps.max() <= 8
        n_multi = int((steps >= 2).sum())
        assert len(order) - n_multi >= 4096 and not (steps[n_multi:] >= 2).any()
    a_val = g.values(c)
    Aq = ops.Csr(g.rowptr, g.col, ops.fake_quantize(_dev(a_val), 0, bits, c.a_s, c.a_z), g.n, plan)
    Xh, W = Q.features(g.n, M, c, 77, dense=True), Q.weights(M, P, c, P)
    X, Wt = _dev(Xh), _dev(W.T)
    fused = ops.layer_forward(Aq, X, Wt, relu=True, quant=c, adj_quantized=True)
    H = chain_H(X, Wt, c)
    chain = ops.spmm(Aq, H, relu=True) * Q.deq32(c)
    assert torch.equal(fused, chain), f"{int((fused != chain).sum())} elements differ from the unfused chain"
    if tail:
        with _lib.tuning(SGX_SPMM_NO_SHORT_TAIL="1"):
            assert torch.equal(ops.layer_forward(Aq, X, Wt, relu=True, quant=c, adj_quantized=True), fused)
    Href, mag, facts = Q.stage1(Xh, W, c)
    Hh = H.cpu().numpy()
    Q.check_H(Hh, Href, mag)
    aq = Q.quantise_adj(a_val, c)
    assert np.array_equal(aq, Aq.val.cpu().numpy())
    D, bound = Q.stage2_gcn((g.rp, g.colh), aq, Hh, c, relu=True)
    Q.check_D(fused.cpu().numpy(), D, bound, {3: "hub row", 100: "row of 65", 101: "row of 200"})
    Q.assert_edges(dict(H=Href, facts=facts, aq=aq), c, adj=(g.rp, g.colh), a_val=a_val, clip_terms=M)
    assert (g.degs == 0).any() and not fused[_dev(g.degs == 0, torch.bool)].any()
    assert (fused < 0).any() if deq else (fused > 0).any()


# ---- stage 2, GAT aggregate -------------------------------------------------------------------------------------------

LONG_ZERO, EMPTY_ROW, ZERO_ROW = 28, 26, 27
NAMES = {20: "row of 300", 21: "row of 600", 22: "row of 257", 23: "row of 256", 24: "row of 65", 25: "row of 64",
         EMPTY_ROW: "empty row", ZERO_ROW: "row quantised to 0", LONG_ZERO: "long row quantised to 0"}


def _gat_degs():
    rng = np.random.default_rng(8)
    degs = rng.integers(0, 9, 8300)
    degs[20:29] = [300, 600, 257, 256, 65, 64, 0, 12, 300]
    return degs


@pytest.fixture(scope="module")
def gat_graph():
    g = _Graph(_gat_degs(), 8)
    g.refs = {}
    return g


def _distinct_forms():
    """FORMS by what reaches the aggregate through the quantised layer: the tuning overrides, the plan and whether E / S are
    wanted.  The entry point is always the layer here and the dead-row rule is one of the two the layer can reach, so
    entries of FORMS that differ only in those are one case, named after all of them.  (SGX_GAT_NO_FUSED_SCORES is left
    out of the key: the X.W score epilogue is fp16-only and off in the quantised layer, so it changes nothing here.)"""
    groups = {}
    for name, (tune, plan_kind, _entry, want_es, _rule) in FORMS.items():
        key = (tuple(sorted((k, v) for k, v in tune.items() if k != "SGX_GAT_NO_FUSED_SCORES")), plan_kind, want_es)
        groups.setdefault(key, []).append(name)
    return [pytest.param(dict(k[0]), k[1], k[2], id="+".join(names)) for k, names in groups.items()]


def _fused_applies(F):
    """sgx_gat_fused_applicable for one fp32 head of F columns on 16-byte aligned rows: the head's F / 4 lanes are a power
    of two and fit the row's lane group."""
    lpr = 1
    while lpr < (F + 3) // 4:
        lpr *= 2
    hl = F // 4
    return F % 4 == 0 and F <= min(lpr, 64) * 4 and hl & (hl - 1) == 0 and hl <= min(lpr, 64)


# (F, w_qbits, the rule for rows without a live entry): both widths, both bit widths and both rules the layer can reach
# (the mean of Wh's rows where the adjacency has dead rows; 0 where the caller's facts say it has none) on every form
@pytest.mark.parametrize("F,bits,rule", [(24, 8, "mean"), (64, 8, "zero"), (64, 2, "mean"), (24, 2, "zero")])
@pytest.mark.parametrize("tune,plan_kind,want_es", _distinct_forms())
def test_stage2_gat_aggregate(gat_graph, tune, plan_kind, want_es, F, bits, rule):
    from sgracex1_amd import _lib, ops
    g, M = gat_graph, 16
    if tune.get("SGX_GAT_FUSED") == "2" and not want_es:
        # the one walk (gat_fused.hip) runs at F = 64 (16 lanes) under both rules and bit widths; at F = 24 a head is 6
        # lanes, sgx_gat_fused_applicable refuses it and the call takes the two stages of its plan, as the "rows" /
        # "ordered_scan" cases do: those ids repeat that path and do not reach gat_fused.hip
        assert _fused_applies(F) == (F == 64)
    c = _constants(bits)
    plan = g.plan(plan_kind) if plan_kind is not None else None           # (asserts the plan facts of its kind)
    a_val = g.values(c, dead_rows=(ZERO_ROW, LONG_ZERO))
    Aq = ops.Csr(g.rowptr, g.col, ops.fake_quantize(_dev(a_val), 0, bits, c.a_s, c.a_z), g.n)
    Aq._plan = Aq._gat_plan = plan
    assert Aq.nnz >= 8192 and Aq.has_dead_rows                            # (8192 entries and more: the planned forms)
    Aq.with_facts(has_dead_rows=(rule == "mean"))                         # what the layer derives its rule from
    Xh, W, att = Q.features(g.n, M, c, 78, dense=True), Q.weights(M, F, c, F), Q.attention(F, c, F)
    X, Wt, att_t = _dev(Xh), _dev(W.T), _dev(att)
    kw = dict(alpha=0.2, relu=True, want_edge_outputs=want_es, use_plan=plan is not None)
    with _lib.tuning(**tune):
        fused = ops.layer_forward(Aq, X, Wt, gat_attention=att_t, quant=c, adj_quantized=True, **kw)
        H = chain_H(X, Wt, c)
        att_q = ops.fake_quantize(att_t, 1, bits, c.w_s, c.w_z)
        chain = ops.gat_aggregate(Aq, H, att_q, fill_dead_rows=(rule == "mean"), **kw)
    if want_es:
        (fused, E, S), (chain, E0, S0) = fused, chain
        assert torch.equal(E, E0) and torch.equal(S, S0)
    chain = chain * Q.deq32(c)
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, chain), f"{int((fused != chain).sum())} elements differ from the unfused chain"
    key = (F, bits, rule)
    if key not in g.refs:
        Href, mag, facts = Q.stage1(Xh, W, c)
        Hh = H.cpu().numpy()
        Q.check_H(Hh, Href, mag)
        aq = Q.quantise_adj(a_val, c)
        assert np.array_equal(aq, Aq.val.cpu().numpy())
        aqt, _ = Q.quantise(att, 1, c)
        assert np.array_equal(aqt, att_q.cpu().numpy())
        D, bound, ref = Q.stage2_gat((g.rp, g.colh), aq, Hh, aqt, c, True, rule)
        Q.assert_edges(dict(H=Href, facts=facts, aq=aq, dead=ref["dead"]), c, adj=(g.rp, g.colh), a_val=a_val, clip_terms=M,
                       gat_rows=(ZERO_ROW, EMPTY_ROW))
        assert ref["dead"][LONG_ZERO] and np.abs(D).max() > 0
        g.refs[key] = (Hh, D, bound)
    Hh, D, bound = g.refs[key]
    assert np.array_equal(H.cpu().numpy(), Hh)
    Q.check_D(fused.cpu().numpy(), D, bound, NAMES)
