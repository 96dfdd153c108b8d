"""The quantised layer's store epilogue on the entry-split schedule (include/sgx.h: sgx_spmm_csr_flat_ep,
sgx_gat_aggregate_flat_ep, SGX_QUANT_FLAT), from the kernels up to the loader.

1. aggregation: on tests/_spmm_flat_ref.degree_cases(T) -- rows inside a chunk, across one chunk end, hub rows over several
   chunks, cooperative pieces, empty first and last rows, capacities past the count -- spmm(out_scale=s) is spmm() times s
   and spmm(requant=) is requantize_ of spmm(), bit for bit (fp32: every step is one IEEE operation); fp16 ignores out_scale,
   the row kernels' rule.
2. GAT: the same graphs with a dead hub row and a dead short row, the three dead-row rules, with and without statistics:
   D is the unscaled D times s, the statistics are the unscaled call's.
3. layer: sgx_layer_forward with SGX_QUANT_FLAT equals the named stage calls composed, bit for bit, and lies inside the
   float64 bounds of tests/_quant_ref.py (stage2_gcn / stage2_gat: _spmm_acc_ref's and _gat_ref's bounds times deq_o) on the
   quantised operands.  No tolerance of its own.
4. model and loader: NeighborLoader(pad=True, schedule="flat", quant=, flat_quant=True) at fan-outs [80, 4]; a padded batch
   against the same matrices at their exact counts; replayed epochs and evaluation passes against eager ones."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import _quant_ref as Q
import _spmm_acc_ref as SA
import _spmm_flat_ref as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA = 0.2
N_COLS = 230                              # at least the rows of every degree case (the GAT form wants n_cols >= n_rows)


@functools.lru_cache(maxsize=None)
def T():
    from sgracex1_amd import _lib
    t = _lib.lib.sgx_spmm_flat_chunk()
    assert t == 256
    return t


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def constants(nbits):
    from sgracex1_amd import quant
    return quant.constants(nbits)


def csr(rp, ci, va, n_cols, dtype=torch.float32, capacity=None, **facts):
    """the matrix on the device; capacity: col / val that long, with what lies behind the end never to be read"""
    from sgracex1_amd import ops
    cap = len(ci) if capacity is None else capacity
    col = torch.full((max(cap, 1),), 1 << 30, dtype=torch.int32, device=DEV)
    val = torch.full((max(cap, 1),), float("nan"), dtype=dtype, device=DEV)
    col[:len(ci)] = torch.as_tensor(np.asarray(ci, np.int32))
    val[:len(ci)] = torch.as_tensor(np.asarray(va)).to(dtype)
    A = ops.Csr(torch.as_tensor(np.asarray(rp, np.int32), device=DEV), col[:cap], val[:cap], n_cols)
    return A.with_facts(**facts) if facts else A


# ---- 1. the aggregation epilogue ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def degree_graphs(dt):
    """name -> (rowptr, col, val, capacity): every degree case at its count, and at a capacity of more than one chunk past
    it (the cases that name one keep theirs)"""
    out = {}
    for k, (name, (deg, cap)) in enumerate(F.degree_cases(T()).items()):
        assert len(deg) <= N_COLS
        rp, ci, va = F.build(deg, N_COLS, dt, seed=k)
        out[name] = (rp, ci, va, cap if cap else len(ci))
        if not cap:
            out[name + "+cap"] = (rp, ci, va, len(ci) + T() + 37)
    return out


def table(n_feat, dt, seed=0):
    """H [N_COLS, n_feat] with entries up to +-4: the sums of short rows land where the 4-bit rule rounds at ties (|x / 8|
    in [0.42, 0.84): x 10^7 has a last bit of one half in fp32), those of hub rows far past both clip bounds"""
    rng = np.random.default_rng([n_feat, seed])
    H = SA.rounded(rng.uniform(-4.0, 4.0, (N_COLS, n_feat)), dt)
    return torch.as_tensor(H).to(torch.float16 if dt == "f16" else torch.float32).to(DEV)


def requant_facts(D0, qc):
    """how many elements of the unscaled D the rule clips, and how many it rounds at an exact tie -- on the rule's own fp32
    steps (sgx_requantize: x / 2^scale_fea, clip, rint(v 10^(ib - 1)) / 10^(ib - 1))"""
    ib = qc.internal_quantization
    v = (D0.float().cpu().numpy() * np.float32(1.0 / 2 ** qc.scale_fea)).astype(np.float32)
    bound = np.float32((2 ** ib - 1) / 2 ** ib)
    clipped = int((np.abs(v) > bound).sum())
    t = (np.clip(v, -bound, bound) * np.float32(10.0 ** (ib - 1))).astype(np.float32)
    return clipped, int((np.abs(t - np.trunc(t)) == 0.5).sum())


@pytest.mark.parametrize("n_feat", [1, 3, 64, 100])
def test_aggregation_epilogue(n_feat):
    from sgracex1_amd import ops
    H = table(n_feat, "f32")
    seen = dict(crossing=0, hub=0, coop=0, clipped=0, ties=0)
    for name, (rp, ci, va, cap) in degree_graphs("f32").items():
        deg = np.diff(rp)
        sch = F.schedule(rp, T(), cap)
        seen["crossing"] += len(sch.sums)
        seen["hub"] += sum(len(v) > 3 for v in sch.sums.values())
        seen["coop"] += sum(e1 - e0 >= 64 for _, _, e0, e1 in sch.reads)
        assert name != "empty_first_last" or (deg[0] == 0 and deg[-1] == 0)
        for relu in (False, True):
            A = csr(rp, ci, va, N_COLS, capacity=cap)
            D0 = ops.spmm(A, H, relu=relu, schedule="flat")
            for qc in (constants(8), constants(4)):
                what = (name, n_feat, relu, qc.w_qbits)
                s = float(np.float32(qc.deq_o))
                assert same(ops.spmm(A, H, relu=relu, schedule="flat", out_scale=s), D0 * s), what
                rq = (qc.scale_fea, qc.internal_quantization)
                want = ops.requantize_(D0.clone(), *rq)
                assert same(ops.spmm(A, H, relu=relu, schedule="flat", requant=rq), want), what
                assert same(ops.spmm(A, H, relu=relu, schedule="flat", requant=rq, out_scale=s), want * s), what
                if not relu and qc.w_qbits == 4:
                    c, t = requant_facts(D0, qc)
                    seen["clipped"] += c
                    seen["ties"] += t
            assert same(ops.spmm(A, H, relu=relu, schedule="flat", out_scale=-0.75), D0 * -0.75), (name, n_feat, relu)
    # the edges the cases are there for did occur (on the schedule's and the rule's own numbers)
    assert seen["crossing"] >= 10 and seen["hub"] >= 4 and seen["coop"] >= 10, seen
    assert seen["clipped"] > 0 and seen["ties"] > 0, seen


@pytest.mark.parametrize("n_feat", [3, 64])
def test_aggregation_out_scale_on_fp16_is_the_row_kernels_rule(n_feat):
    """sgx_epilogue: "fp16 instantiations ignore it" -- out_scale leaves an fp16 D as it is; requantising is fp32-only"""
    from sgracex1_amd import ops
    H = table(n_feat, "f16")
    for name, (rp, ci, va, cap) in degree_graphs("f16").items():
        A = csr(rp, ci, va, N_COLS, dtype=torch.float16, capacity=cap)
        for relu in (False, True):
            D0 = ops.spmm(A, H, relu=relu, schedule="flat")
            assert same(ops.spmm(A, H, relu=relu, schedule="flat", out_scale=2.5), D0), (name, n_feat, relu)
    with pytest.raises(TypeError, match="requant works on float32"):
        ops.spmm(A, H, schedule="flat", requant=(4, 16))


# ---- 2. the GAT epilogue --------------------------------------------------------------------------------------------------------

def masked(rp, va, seed):
    """a fifth of the stored values <= 0 (masked); the longest row (a hub row where the case has one) and the first other
    row of 1 to 12 entries lose every positive value (dead): the hub's to negative ones, the short row's to 0"""
    rng = np.random.default_rng([seed, 9])
    va = np.array(va, np.float64)
    va[rng.random(len(va)) < 0.2] *= -1
    deg = np.diff(rp)
    dead = []
    if deg.max() > 0:
        hub = int(np.argmax(deg))
        va[rp[hub]:rp[hub + 1]] = -np.abs(va[rp[hub]:rp[hub + 1]])
        dead.append(hub)
        short = [r for r in range(len(deg)) if 1 <= deg[r] <= 12 and r != hub]
        if short:
            va[rp[short[0]]:rp[short[0] + 1]] = 0.0
            dead.append(short[0])
    return va, dead


@pytest.mark.parametrize("n_feat", [3, 64])
def test_gat_epilogue(n_feat):
    from sgracex1_amd import ops
    Wh = table(n_feat, "f32", seed=1) * 0.25
    rng = np.random.default_rng(n_feat)
    att = torch.as_tensor(rng.standard_normal(2 * n_feat) / np.sqrt(n_feat), dtype=torch.float32, device=DEV)
    fill_row = torch.as_tensor(rng.standard_normal(n_feat), dtype=torch.float32, device=DEV)
    s = float(np.float32(constants(8).deq_o))
    dead_hubs = dead_short = 0
    for k, (name, (rp, ci, va, cap)) in enumerate(degree_graphs("f32").items()):
        va, dead = masked(rp, va, k)
        deg = np.diff(rp)
        dead_hubs += sum(deg[r] > T() for r in dead)
        dead_short += sum(deg[r] <= 12 for r in dead)
        A = csr(rp, ci, va, N_COLS, capacity=cap)
        for relu in (False, True):
            for rule in (dict(fill_dead_rows=False), dict(fill_dead_rows=True), dict(fill_row=fill_row, n_nodes=1000)):
                what = (name, n_feat, relu, sorted(rule))
                kw = dict(alpha=ALPHA, relu=relu, schedule="flat", **rule)
                D0, st0 = ops.gat_aggregate(A, Wh, att, want_row_stats=True, **kw)
                D1, st1 = ops.gat_aggregate(A, Wh, att, want_row_stats=True, out_scale=s, **kw)
                assert same(D1, D0 * s), what
                assert all(same(a, b) for a, b in zip(st1.tensors(), st0.tensors())), what
                assert same(ops.gat_aggregate(A, Wh, att, out_scale=s, **kw), D1), what        # without statistics: the same D
                for r in dead:
                    assert float(st0.row_sum[r]) == 0.0 and float(st0.row_max[r]) == 0.0, what
                if dead and "fill_row" in rule:
                    want = (torch.relu(fill_row) if relu else fill_row) * s
                    assert same(D1[dead[0]], want), what                                      # the dead row's fill takes out_scale too
    assert dead_hubs >= 4 and dead_short >= 10
    A16 = csr(rp, ci, va, N_COLS, dtype=torch.float16, capacity=cap)
    D0 = ops.gat_aggregate(A16, Wh.half(), att.half(), alpha=ALPHA, schedule="flat", fill_dead_rows=True)
    assert same(ops.gat_aggregate(A16, Wh.half(), att.half(), alpha=ALPHA, schedule="flat", fill_dead_rows=True, out_scale=s), D0)


# ---- 3. the layer ---------------------------------------------------------------------------------------------------------------

N_ROWS, L_COLS, LONG, DEADQ = 300, 320, 1, 4
FORMS = {"dense32": (32, 20), "dense144-int8": (144, 32), "csr-rows": (40, 20), "csr-flat": (40, 20)}      # M_fea, P


@functools.lru_cache(maxsize=None)
def layer_case(nbits, form):
    """about 300 rows, row 1 of 700 entries (three chunk ends), row 4's every stored value under half a step of the
    adjacency grid: it dies under the QUANTISED mask only; operands over the quantiser's ranges and past them"""
    c = constants(nbits)
    M, P = FORMS[form]
    rng = np.random.default_rng([nbits, M])
    degs = list(rng.poisson(5.0, N_ROWS))
    degs[0], degs[LONG], degs[2], degs[DEADQ], degs[-1] = 0, 700, 3, 6, 0
    rp, ci, va = Q.adjacency(degs, L_COLS, c, seed=nbits, dead_rows=(DEADQ,))
    assert (va[rp[DEADQ]:rp[DEADQ + 1]] > 0).all() and not (Q.quantise_adj(va, c)[rp[DEADQ]:rp[DEADQ + 1]] > 0).any()
    X = Q.features(L_COLS, M, c, seed=nbits + 1, dense=True)
    W = Q.weights(M, P, c, seed=nbits + 2)
    att = Q.attention(P, c, seed=nbits + 3)
    return c, (rp, ci, va), X, W, att


def stage1(form, c, X, Wt):
    """H = requant(X_q . W_q) by the named stage calls, into rows of the layer's pitch -> (H [n, ldh], the feature operand
    the layer call takes)"""
    from sgracex1_amd import ops
    P, M = Wt.shape
    ldh = ops.table_pitch(P, 4)
    rq = (c.scale_fea, c.internal_quantization)
    H = torch.zeros((X.shape[0], ldh), dtype=torch.float32, device=DEV)
    if form == "dense144-int8":
        Xc, _ = ops.quantize_codes_i8(X, 0, c.w_qbits, c.f_s, c.f_z)
        Wc, _ = ops.quantize_codes_i8(Wt, 1, c.w_qbits, c.w_s, c.w_z)
        H[:, :P] = ops.xw_dense_i8(Xc, Wc, M, c.w_qbits, *rq)
        return H, X
    Bq = ops.fake_quantize(Wt, 1, c.w_qbits, c.w_s, c.w_z)
    if form == "dense32":
        Xq = ops.fake_quantize(X, 0, c.w_qbits, c.f_s, c.f_z)
        H[:, :P] = ops.xw_dense(Xq, Bq, ldh=ldh)[:, :P]
        ops.requantize_(H[:, :P], *rq)
        return H, X
    Xc = ops.Csr.from_dense(X)
    Xq = ops.Csr(Xc.rowptr, Xc.col, ops.fake_quantize(Xc.val, 0, c.w_qbits, c.f_s, c.f_z), Xc.n_cols)
    W = ops.transpose(Bq, ldo=ldh)
    if form == "csr-rows":
        ops.xw_sparse(Xq, W[:, :P], out=H[:, :P], use_plan=False)        # (as the descriptor below: no plan_fea)
    else:
        ops.spmm(Xq, W, n_feat=P, out=H[:, :P], schedule="flat")
        Xc = Xc.with_facts(flat=True, flat_quant=True)
    ops.requantize_(H[:, :P], *rq)
    return H, Xc


def direct_layer(A, fea, Wt, c, relu, att, fill, adj_done, stats):
    """sgx_layer_forward[_stats] on a descriptor built here: SGX_SCHEDULE_FLAT at the capacity A.col holds, SGX_QUANT_FLAT,
    SGX_QUANT_INT8_AUTO (what config.hardware_quantize selects; the integer form from 129 columns on)"""
    from sgracex1_amd import _lib, ops
    P, M = Wt.shape
    sparse = isinstance(fea, ops.Csr)
    d = _lib.LayerDesc(gemm_mode=0 if sparse else 1, relu=int(relu), gat_mode=int(att is not None), N_adj=A.n_rows, M_adj=A.n_cols,
                       M_fea=M, P_w=P, dtype=ops.dtype_code(Wt.dtype), spmm_block=1, fea_threads=1, adj_threads=1,
                       gat_fill_dead_rows=int(fill), alpha=ALPHA, B=Wt.data_ptr(), rowPtr_adj=A.rowptr.data_ptr(),
                       columnIndex_adj=A.col.data_ptr(), values_adj=A.val.data_ptr(), schedule_adj=_lib.SGX_SCHEDULE_FLAT,
                       nnz_adj=A.nnz)
    if sparse:
        d.rowPtr_fea, d.columnIndex_fea, d.values_fea = fea.rowptr.data_ptr(), fea.col.data_ptr(), fea.val.data_ptr()
    else:
        d.values_fea = fea.data_ptr()
    if att is not None:
        d.attention, d.gat_heads = att.data_ptr(), 1
    qs = c.as_struct(nnz_adj=A.nnz, nnz_fea=fea.nnz if sparse else 0, adj_done=adj_done)
    qs.flags |= _lib.SGX_QUANT_FLAT | _lib.SGX_QUANT_INT8_AUTO
    d.quant = ctypes.pointer(qs)
    assert _lib.lib.sgx_layer_schedule(ctypes.byref(d)) == 2
    D = torch.full((A.n_rows, P), float("nan"), dtype=torch.float32, device=DEV)
    d.D = D.data_ptr()
    nbytes = _lib.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    d.workspace, d.workspace_bytes = ws.data_ptr() + (-ws.data_ptr()) % 256, nbytes
    stream = torch.cuda.current_stream().cuda_stream
    if stats:
        st = ops.GatStats(A.n_rows, A.n_cols, 1, torch.device(DEV))
        ss = st.struct()
        ops.check(_lib.lib.sgx_layer_forward_stats(ctypes.byref(d), ctypes.byref(ss), stream), "sgx_layer_forward_stats")
        return D, st
    ops.check(_lib.lib.sgx_layer_forward(ctypes.byref(d), stream), "sgx_layer_forward")
    return D, None


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("nbits", [8, 4])
@pytest.mark.parametrize("gat", [0, 1], ids=["gcn", "att"])
def test_layer_equals_the_stage_calls_composed(gat, nbits, form):
    from sgracex1_amd import ops
    c, (rp, ci, va), X_h, W_h, att_h = layer_case(nbits, form)
    X = torch.as_tensor(X_h, device=DEV)
    Wt = torch.as_tensor(np.ascontiguousarray(W_h.T), device=DEV)
    att = torch.as_tensor(att_h, device=DEV) if gat else None
    H, fea = stage1(form, c, X, Wt)
    P = Wt.shape[0]
    deq = float(np.float32(c.deq_o))
    att_q = ops.fake_quantize(att, 1, c.w_qbits, c.w_s, c.w_z) if gat else None
    aq_h = Q.quantise_adj(va, c)
    H_h = H[:, :P].cpu().numpy()
    for cap in (len(ci), len(ci) + 2 * T() + 5):
        A = csr(rp, ci, va, L_COLS, capacity=cap)
        Aq = csr(rp, ci, va, L_COLS, capacity=cap)
        ops.fake_quantize(Aq.val, 0, c.w_qbits, c.a_s, c.a_z, out=Aq.val)                 # (the whole capacity, as the layer does)
        assert np.array_equal(Aq.val[:len(ci)].cpu().numpy(), aq_h)
        for relu in (False, True):
            for fill in ((0, 1) if gat else (0,)):
                what = (gat, nbits, form, cap - len(ci), relu, fill)
                if gat:
                    want, wst = ops.gat_aggregate(Aq, H[:, :P], att_q, alpha=ALPHA, relu=relu, fill_dead_rows=bool(fill),
                                                  want_row_stats=True, schedule="flat", out_scale=deq)
                else:
                    want, wst = ops.spmm(Aq, H, relu=relu, n_feat=P, schedule="flat", out_scale=deq), None
                got = []
                if form == "csr-flat":
                    # no C entry takes an H formed elsewhere: the layer is ops.layer_forward's composition on the pair of facts
                    for done in (False, True):
                        Am = (Aq if done else A).with_facts(flat=True, flat_quant=True)
                        kw = dict(gat_attention=att, alpha=ALPHA, fill_dead_rows=bool(fill)) if gat else {}
                        assert ops.layer_schedule(Am, fea, Wt, relu=relu, quant=c, adj_quantized=done, **kw) == 2
                        got.append((ops.layer_forward(Am, fea, Wt, relu=relu, quant=c, adj_quantized=done, **kw), None))
                        if gat:
                            got.append(ops.layer_forward(Am, fea, Wt, relu=relu, quant=c, adj_quantized=done, want_row_stats=True, **kw))
                else:
                    for done in (False, True):
                        for stats in ((False, True) if gat else (False,)):
                            got.append(direct_layer(Aq if done else A, fea, Wt, c, relu, att, fill, done, stats))
                    # and through ops: the keyword with its opt-in
                    kw = dict(gat_attention=att, alpha=ALPHA, fill_dead_rows=bool(fill)) if gat else {}
                    got.append((ops.layer_forward(A, fea, Wt, relu=relu, quant=c, quant_int8="auto", schedule="flat", quant_flat=True,
                                                  use_plan=False, **kw), None))
                for D, st in got:
                    assert same(D, want), what
                    if st is not None:
                        assert all(same(a, b) for a, b in zip(st.tensors(), wst.tensors())), what
                # inside the float64 bound on the quantised operands
                if gat:
                    ref, bound, r = Q.stage2_gat((rp, ci), aq_h, H_h, att_q.cpu().numpy(), c, relu, "mean" if fill else "zero", alpha=ALPHA)
                    assert r["dead"][DEADQ] and r["dead"][0] and not r["dead"][LONG], what
                    if not fill:
                        assert not bits(want[DEADQ]).any() and not bits(want[0]).any(), what        # dead under the quantised mask: +0
                    assert float(wst.row_sum[DEADQ]) == 0.0 and float(wst.row_max[DEADQ]) == 0.0
                else:
                    ref, bound = Q.stage2_gcn((rp, ci), aq_h, H_h, c, relu)
                Q.check_D(want.cpu().numpy(), ref, bound)
    # without the opt-in the keyword is refused and a flat-marked adjacency runs by rows, as before
    with pytest.raises(ValueError, match="entry-split schedule does not go with .*quant"):
        ops.layer_forward(A, X if form.startswith("dense") else ops.Csr.from_dense(X), Wt, quant=c, schedule="flat")
    if form.startswith("dense"):
        marked = csr(rp, ci, va, L_COLS, flat=True)
        assert ops.layer_schedule(marked, X, Wt, quant=c) in (0, 1)
        assert ops.layer_schedule(marked.with_facts(flat_quant=True), X, Wt, quant=c) == 2


# ---- 4. model and loader --------------------------------------------------------------------------------------------------------

N, HUB, WIDTH, BATCH, FAN, SEEDS = 300, 7, 40, 32, [80, 4], 72
MODELS = {"gcn-emu": (0, 0, 1), "gcn-hw": (0, 1, 1), "att-emu-edges": (1, 0, 1), "att-emu-lean": (1, 0, 0), "att-hw-edges": (1, 1, 1),
          "att-hw-lean": (1, 1, 0)}                                         # attention, hardware_quantize, gat_edge_outputs


def _data():
    from sgracex1_amd import pyg_lite
    rng = np.random.default_rng(3)
    m = rng.random((N, N)) < 0.02
    near = rng.choice(N, 250, replace=False)
    m[near, HUB] = True
    m[HUB, near] = True
    np.fill_diagonal(m, False)
    src, dst = np.nonzero(m)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((N, WIDTH), generator=g) < 0.25).float() * torch.rand((N, WIDTH), generator=g)
    y = (torch.arange(N) * 7 % 5).to(DEV)
    train = torch.zeros(N, dtype=torch.bool, device=DEV)
    train[torch.randperm(N, generator=torch.Generator().manual_seed(2))[:SEEDS - 1].to(DEV)] = True
    train[HUB] = True
    assert int(train.sum()) in (SEEDS - 1, SEEDS)
    return pyg_lite.NodeData(x.to(DEV).contiguous(), torch.as_tensor(np.stack([src, dst])).to(DEV), y, train_mask=train)


@pytest.fixture
def env(request):
    from sgracex1_amd import config, sgrace
    gat, hwq, edges = MODELS[request.param]
    saved = config.snapshot()
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, gat
    config.fake_quantization, config.hardware_quantize = 1, hwq
    config.w_qbits, config.gat_edge_outputs, config.device = 8, edges, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(5)
    data = _data()
    model = sgrace.GAT_PYNQ(WIDTH, 16, 1, 5).to(DEV).train()
    kw = dict(batch_size=BATCH, input_nodes=data.train_mask, shuffle=True, seed=3, prepare="sym_norm2", fill=1 if gat else 0,
              dtype=torch.float32, transposed=True, pad=True, schedule="flat", quant=sgrace.quant_constants, flat_quant=True)
    yield model, data, gat, kw
    config.restore(saved)
    sgrace.init_SGRACE()


@pytest.mark.parametrize("env", list(MODELS), indirect=True)
def test_padded_batch_equals_the_same_draw_at_its_exact_counts(env, monkeypatch):
    """the same bits at every capacity: the padded batch against the same draw unpadded -- the same live matrices with nnz at
    their counts (tests/test_gpu_node_pad_flat.py holds the padded arrays to them) under the same facts"""
    from sgracex1_amd import ops, pyg_lite, sgrace
    model, data, gat, kw = env
    qc = sgrace.quant_constants
    loader = pyg_lite.NeighborLoader(data, FAN, **kw)
    assert loader.capacity.max_row == 81
    seeds, input_id, step = next(iter(loader.epoch_batches()))
    assert loader.padded(seeds)
    u = loader._prepared(seeds, input_id, step)
    live = u.num_real_nodes
    for M in [u.adj_norm] + list(u.adj_norm._quantized.values()):     # the padded batch's constant fact: the same kernel path
        M.with_facts(has_dead_rows=True)
    loader.load(seeds, step)
    p = loader.padded_batch(input_id)
    loader.status()
    A = p.adj_norm
    n = p.x.shape[0]
    for M, U in ((A, u.adj_norm), (ops.recorded(p.x, ("fea_csr", torch.float32)), ops.recorded(u.x, ("fea_csr", torch.float32)))):
        k = U.nnz
        assert U._flat and U._flat_quant and same(M.rowptr[:live + 1], U.rowptr) and k < M.nnz
        assert same(M.col[:k], U.col[:k]) and same(M.val[:k], U.val[:k])
    assert int((A.rowptr[1:] - A.rowptr[:-1]).max()) == 81              # the hub's row: past what a row schedule pads
    mats = [A, ops.recorded(p.x, ("fea_csr", torch.float32)), A._transpose_pattern[0], ops.recorded(p.x, ("fea_csr_t", torch.float32))]
    mats += list(A._quantized.values()) + [Qm._lean_values for Qm in A._quantized.values()]
    assert set(A._quantized) == {ops._adj_quant_key(qc), ops._adj_quant_key(qc.second_layer())}
    assert all(M._flat and M._flat_quant and not M.wants_plan and M._plan is None for M in mats)
    # both layers take the entry-split schedule
    fea = ops.recorded(p.x, ("fea_csr", torch.float32))
    att1 = dict(gat_attention=model.att2.attention.detach().reshape(-1).contiguous(), fill_dead_rows=True) if gat else {}
    att2 = dict(gat_attention=model.conv22.attention.detach().reshape(-1).contiguous(), fill_dead_rows=True) if gat else {}
    assert ops.layer_schedule(A, fea, model.att2.weight.detach().t().contiguous(), quant=qc, **att1) == 2
    hidden = torch.zeros((n, model.conv22.weight.shape[0]), device=DEV)
    assert ops.layer_schedule(A, hidden, model.conv22.weight.detach().t().contiguous(), quant=qc.second_layer(), **att2) == 2
    built = []
    plan_init = ops.Plan.__init__
    monkeypatch.setattr(ops.Plan, "__init__", lambda self, *a, **k: (built.append(a), plan_init(self, *a, **k))[1])

    def run(b):
        for q in model.parameters():
            q.grad = None
        Hm = model.features(b.x, b.edge_index_agg).contiguous()
        loss = ops.NodeLoss.apply(Hm, model.lin.weight, model.lin.bias, b.y, None, BATCH, 0.0, 0, 0, None)
        loss.backward()
        return Hm.detach().clone(), loss.detach().reshape(1).clone(), {k: None if q.grad is None else q.grad.clone()
                                                                       for k, q in model.named_parameters()}

    H_e, loss_e, g_e = run(u)
    H_p, loss_p, g_p = run(p)
    assert not built, f"{len(built)} plans were built"
    assert live == int(loader.counts[0]) < n and bool(H_e.any()) and bool(torch.isfinite(H_p).all())
    assert same(H_p[:live], H_e), "live rows"
    assert not H_p[live:].any(), "filler rows"
    assert same(loss_p, loss_e)
    assert [k for k in g_p if g_p[k] is None] == [k for k in g_e if g_e[k] is None]
    for k in g_p:
        if g_p[k] is not None:
            print(k, "bit-equal" if same(g_p[k], g_e[k]) else "not bit-equal", "max |padded - exact|",
                  float((g_p[k] - g_e[k]).abs().max()), "max |exact|", float(g_e[k].abs().max()))
            assert same(g_p[k], g_e[k]), k
    for k in ["att2.weight", "conv22.weight"] + (["att2.attention", "conv22.attention"] if gat else []):
        assert bool(g_p[k].any()), k                                    # a gradient did arrive


@pytest.mark.parametrize("env", ["gcn-hw", "att-hw-edges", "att-emu-lean"], indirect=True)
def test_replayed_epochs_equal_eager_steps(env, monkeypatch):
    from sgracex1_amd import ops, pyg_lite
    from sgracex1_amd.train import NodeTrainer
    model, data, gat, kw = env
    twin = copy.deepcopy(model)
    a, b = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5), NodeTrainer(twin, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = pyg_lite.NeighborLoader(data, FAN, **kw), pyg_lite.NeighborLoader(data, FAN, **kw)
    assert len(la) == 3 and len(la.buffers.quant) == 1
    epoch = a.capture_loader(la)
    assert int(a.t) == 0
    built = []
    plan_init = ops.Plan.__init__
    monkeypatch.setattr(ops.Plan, "__init__", lambda self, *a_, **k: (built.append(a_), plan_init(self, *a_, **k))[1])
    replayed = []
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                             # a replayed epoch reads nothing back through torch
    try:
        for _ in range(2):
            replayed += epoch()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    monkeypatch.undo()
    assert not built, f"{len(built)} plans were built during the replayed epochs"
    eager = [b.step(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size) for _ in range(2) for bt in lb]
    la.status(), lb.status()
    assert len(replayed) == len(eager) == 2 * len(la) == 6
    for i, (r, e) in enumerate(zip(replayed, eager)):
        assert same(r, e), i
        assert bool(torch.isfinite(r).all())
    assert int(a.t) == int(b.t) == 2 * len(la)
    for x1, x2 in zip(a.state(), b.state()):
        assert same(x1, x2)


@pytest.mark.parametrize("env", ["gcn-hw", "att-hw-edges"], indirect=True)
def test_captured_eval_pass_equals_the_eager_pass(env):
    from sgracex1_amd import pyg_lite
    from sgracex1_amd.train import EvalSums, NodeTrainer
    model, data, gat, kw = env
    kw = dict(kw, shuffle=False)
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = pyg_lite.NeighborLoader(data, FAN, **kw), pyg_lite.NeighborLoader(data, FAN, **kw)
    state = trainer.state()
    run_pass = trainer.capture_eval_loader(la)
    replayed = [run_pass().buffer.clone() for _ in range(2)]
    eager, sums = [], EvalSums(DEV)
    for _ in range(2):
        sums.zero_()
        for bt in lb:
            trainer.evaluate(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size, into=sums)
        eager.append(sums.buffer.clone())
    la.status(), lb.status()
    for r, e in zip(replayed, eager):
        assert same(r, e) and int(r[0]) == int(data.train_mask.sum())
    assert all(same(x, y) for x, y in zip(state, trainer.state())) and model.training
