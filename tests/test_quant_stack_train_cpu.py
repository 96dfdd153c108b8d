"""sgx_quant_stack_backward without a GPU: symbols, struct layouts, argument errors, the LDS and workspace formulas, and the
float64 restatement the GPU tests compare against (tests/_quant_stack_grad_ref.py) checked against torch.autograd through
the model's dense emulation (config.acc = 0, fake_quantization = 1, FPYNQ_GAT's own backward) and against three mutants
of itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _quant_ref as Q
from test_gat_stack_train_cpu import lds_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

NEW = ["sgx_quant_stack_backward_workspace_bytes", "sgx_quant_stack_backward_lds_bytes", "sgx_quant_stack_backward"]
ADJ_DONE = 1


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_new_symbols_are_exported_and_the_version_stays(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in NEW:
        assert name in L.SYMBOLS
        assert f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110


def test_quant_grad_structs_match_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof_layer %zu\\n", sizeof(sgx_quant_stack_grad_layer));\n'
        ' printf("sizeof_desc %zu\\n", sizeof(sgx_quant_stack_grad_desc));\n'
        + "".join(f' printf("l.{n} %zu\\n", offsetof(sgx_quant_stack_grad_layer, {n}));\n' for n, _ in L.QuantStackGradLayer._fields_)
        + "".join(f' printf("d.{n} %zu\\n", offsetof(sgx_quant_stack_grad_desc, {n}));\n' for n, _ in L.QuantStackGradDesc._fields_)
        + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        seen += 1
        if name == "sizeof_layer":
            assert ctypes.sizeof(L.QuantStackGradLayer) == int(val)
        elif name == "sizeof_desc":
            assert ctypes.sizeof(L.QuantStackGradDesc) == int(val)
        elif name.startswith("l."):
            assert getattr(L.QuantStackGradLayer, name[2:]).offset == int(val), name
        else:
            assert getattr(L.QuantStackGradDesc, name[2:]).offset == int(val), name
    assert seen == 2 + len(L.QuantStackGradLayer._fields_) + len(L.QuantStackGradDesc._fields_)
    # sgx_gat_stack_grad_layer / _desc field for field, then quant / values_adj_q
    assert [n for n, _ in L.QuantStackGradLayer._fields_] == [n for n, _ in L.GatStackGradLayer._fields_] + ["quant"]
    assert [n for n, _ in L.QuantStackGradDesc._fields_] == [n for n, _ in L.GatStackGradDesc._fields_] + ["values_adj_q"]
    for n, _ in L.GatStackGradLayer._fields_:
        assert getattr(L.QuantStackGradLayer, n).offset == getattr(L.GatStackGradLayer, n).offset
    for n, _ in L.GatStackGradDesc._fields_:
        if n not in ("layer",) and getattr(L.GatStackGradDesc, n).offset < L.GatStackGradDesc.layer.offset:
            assert getattr(L.QuantStackGradDesc, n).offset == getattr(L.GatStackGradDesc, n).offset


def _empty_plan(L, kind, width=64, dtype=1):
    h = ctypes.c_void_p()
    assert L.lib.sgx_batch_plan_create_ex(dtype, 0, 0, None, None, None, width, kind, ctypes.byref(h), None) == 0 and h.value
    return h


def _quant(L, bits=8, flags=0):
    from sgracex1_amd import quant
    q = quant.constants(bits).as_struct(nnz_adj=0)
    q.flags = flags
    return q


def _qdesc(L, n_layers=2, gat=(1, 1, 1, 1), dtype=1, width=8, quants=None):
    d = L.QuantStackGradDesc()
    d.dtype, d.n_layers = dtype, n_layers
    for l in range(4):
        d.layer[l].gemm_mode, d.layer[l].M_fea, d.layer[l].P_w = 1, width, width
        d.layer[l].W, d.layer[l].grad_W = 256, 512
        d.layer[l].gat_mode, d.layer[l].attention, d.layer[l].grad_attention, d.layer[l].alpha = gat[l], 768, 1024, 0.2
        if quants is not None and quants[l] is not None:
            d.layer[l].quant = ctypes.pointer(quants[l])
    return d


def test_backward_argument_errors_need_no_gpu(L):
    lib = L.lib
    bwd = lambda d: lib.sgx_quant_stack_backward(ctypes.byref(d), None)
    ws = lambda d: lib.sgx_quant_stack_backward_workspace_bytes(ctypes.byref(d))
    lds = lambda d: lib.sgx_quant_stack_backward_lds_bytes(ctypes.byref(d))
    assert lib.sgx_quant_stack_backward(None, None) == -1                    # SGX_ERR_NULL
    assert lib.sgx_quant_stack_backward_workspace_bytes(None) == 0
    assert lib.sgx_quant_stack_backward_lds_bytes(None) == 0
    for n in (0, 5):
        assert bwd(_qdesc(L, n)) == -2                                        # SGX_ERR_SHAPE
    d = _qdesc(L)
    assert bwd(d) == -1                                                      # no plan
    d.dtype = 7
    assert bwd(d) == -3
    b, f, b16 = _empty_plan(L, 1), _empty_plan(L, 0), _empty_plan(L, 1, dtype=0)
    qs = [_quant(L) for _ in range(4)]
    try:
        # ---- those of sgx_gat_stack_backward, with and without quantisers
        for quants in (None, qs):
            d = _qdesc(L, quants=quants)
            d.plan = b
            assert ws(d) == 256 * -(-4 * (2 * 64 + 2 * 16) // 256)           # one slice: two 8 x 8 blocks, two of 2 x 8
            assert bwd(d) == -4                                              # no workspace
            d.workspace, d.workspace_bytes = 1 << 20, ws(d) - 4              # too small
            assert bwd(d) == -4
            d.workspace, d.workspace_bytes = (1 << 20) + 16, ws(d)           # not 256-byte aligned
            assert bwd(d) == -7
            d.workspace = 1 << 20
            d.layer[0].W = None
            assert bwd(d) == -1 and ws(d) == 0                               # W missing
            d.layer[0].W = 256
            d.layer[1].grad_W = None
            assert bwd(d) == -1                                              # grad_W missing
            d.layer[1].grad_W = 512
            d.layer[1].M_fea = 9                                             # widths do not chain
            assert bwd(d) == -2
            d.layer[1].M_fea, d.layer[1].gemm_mode = 8, 0                    # CSR input past layer 0
            assert bwd(d) == -3
            d.layer[1].gemm_mode, d.layer[1].ldd = 1, 4                      # ldd < P_w
            assert bwd(d) == -2
            d.layer[1].ldd = 0
            d.n_graphs = 1                                                   # graph count not the plan's
            assert bwd(d) == -2
            d.n_graphs = 0
            d.layer[1].attention = None
            assert bwd(d) == -1 and ws(d) == 0                               # attention missing on a GAT layer
            d.layer[1].attention = 768
            d.layer[0].grad_attention = None
            assert bwd(d) == -1 and ws(d) == 0                               # grad_attention missing
            d.layer[0].gat_mode = 0                                          # ... which a GCN layer does not need
            assert ws(d) > 0
            d.layer[0].gat_mode, d.layer[0].grad_attention = 1, 1024
            for mode in (2, -1):
                d.layer[1].gat_mode = mode
                assert bwd(d) == -3 and ws(d) == 0                           # no such gat_mode
            d.layer[1].gat_mode = 1
            d.plan = f                                                       # a forward-kind plan
            assert bwd(d) == -3 and ws(d) == 0 and lds(d) == 0
            d.plan = b
            d.layer[1].P_w, d.layer[2].M_fea = 65, 65                        # wider than the plan
            assert bwd(d) == -3 and ws(d) == 0
            d.layer[1].P_w = 8
        # ---- the quantiser's own
        d = _qdesc(L, dtype=0, quants=qs)                                    # a quantiser on fp16
        d.plan = b16
        assert bwd(d) == -3 and ws(d) == 0 and lds(d) == 0
        d16 = _qdesc(L, dtype=0)                                             # (fp16 without one is sgx_gat_stack_backward)
        d16.plan = b16
        assert ws(d16) > 0
        d = _qdesc(L, dtype=0, quants=[None, qs[1], None, None])             # ... on one layer is enough
        d.plan = b16
        assert bwd(d) == -3
        for field, bad in (("qbits", (0, 3, 16, -1)), ("scale_fea", (-1, 31)), ("internal_bits", (0, 31))):
            for v in bad:
                q = _quant(L)
                setattr(q, field, v)
                d = _qdesc(L, quants=[qs[0], q, None, None])
                d.plan = b
                assert bwd(d) == -3 and ws(d) == 0 and lds(d) == 0, (field, v)
        for bits in (8, 4, 2, 1):
            d = _qdesc(L, quants=[_quant(L, bits)] * 4)
            d.plan = b
            assert ws(d) > 0 and lds(d) > 0
        q = _quant(L)
        q.zero_adj = 0.5
        d = _qdesc(L, quants=[q, None, None, None])
        d.plan = b
        assert bwd(d) == -3 and ws(d) == 0                                   # zero_adj != 0
        q = _quant(L)
        q.zero_fea = 1.0
        d = _qdesc(L, quants=[q, q, None, None])
        d.plan = b
        assert ws(d) > 0                                                     # zero_fea != 0 is fine on dense layers ...
        d.layer[0].gemm_mode = 0
        assert bwd(d) == -3 and ws(d) == 0                                   # ... and refused on a sparse layer 0
        d = _qdesc(L, quants=[None, q, None, None])
        d.plan = b
        d.layer[0].gemm_mode = 0
        assert ws(d) > 0                                                     # (layer 1 is dense)
        # SGX_QUANT_ADJ_DONE on a GAT layer needs values_adj_q wherever a row is read (the quantisers' checks run before
        # the plan's, so a descriptor with rows shows it on the empty plan: -1 without the values, the plan's -2 with them)
        qd = _quant(L, flags=ADJ_DONE)
        d = _qdesc(L, quants=[qd, qd, None, None])
        d.plan = b
        assert ws(d) > 0                                                     # (an empty batch reads none)
        d.n_rows = 3
        assert bwd(d) == -1 and ws(d) == 0 and lds(d) == 0
        d.values_adj_q = 4096
        assert bwd(d) == -2
        d.values_adj_q = None
        d.layer[0].gat_mode = d.layer[1].gat_mode = 0                        # a GCN layer masks with nothing
        assert bwd(d) == -2
        d = _qdesc(L, quants=[None, qd, None, None])                         # ... one GAT layer with the flag is enough
        d.plan, d.n_rows = b, 3
        assert bwd(d) == -1
    finally:
        for p in (b, f, b16):
            assert lib.sgx_batch_plan_destroy(p) == 0


@pytest.mark.parametrize("width", [1, 7, 64, 65, 252, 256])
def test_lds_and_workspace_are_the_gat_backwards(L, width):
    """The LDS formula is sgx_gat_stack_backward_lds_bytes' (H_q and the unquantised Wh share one tile) and the workspace
    is the same slices, with a quantiser on every layer, on some or on none."""
    lib = L.lib
    p = _empty_plan(L, 1, width, 1)
    qs = [_quant(L, 4) for _ in range(4)]
    try:
        rows, want = lds_bytes(4, width)
        g = L.GatStackGradDesc()
        g.dtype, g.n_layers = 1, 2
        for l in range(4):
            g.layer[l].gemm_mode, g.layer[l].M_fea, g.layer[l].P_w = 1, width, width
            g.layer[l].W, g.layer[l].grad_W = 256, 512
            g.layer[l].gat_mode, g.layer[l].attention, g.layer[l].grad_attention, g.layer[l].alpha = 1, 768, 1024, 0.2
        g.plan = p
        for quants in (qs, [None, qs[1], None, None], None):
            d = _qdesc(L, width=width, quants=quants)
            d.plan = p
            assert lib.sgx_batch_plan_rows(p) == rows
            assert lib.sgx_quant_stack_backward_lds_bytes(ctypes.byref(d)) == want
            assert lib.sgx_quant_stack_backward_lds_bytes(ctypes.byref(d)) == lib.sgx_gat_stack_backward_lds_bytes(ctypes.byref(g))
            assert lib.sgx_quant_stack_backward_workspace_bytes(ctypes.byref(d)) == \
                lib.sgx_gat_stack_backward_workspace_bytes(ctypes.byref(g)) > 0
            assert lib.sgx_quant_stack_backward_workspace_bytes(ctypes.byref(d)) == 256 * -(-4 * 2 * (-(-width * width // 4) * 4 + -(-2 * width // 4) * 4) // 256)
    finally:
        lib.sgx_batch_plan_destroy(p)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------
def _mutag12():
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs[:12])


@pytest.mark.parametrize("gat", [1, 0])
@pytest.mark.parametrize("bits", [8, 2])
def test_restatement_is_autograd_through_the_quantised_dense_emulation(bits, gat):
    """GAT_POOL_PYNQ with config.acc = 0, fake_quantization = 1 on a 12-graph MUTAG batch: torch.autograd through
    FPYNQ_GAT's dense emulation -- the quantised forward, the backward on the unquantised operands -- and RPYNQ, against
    the restatement on the emulation's own layer outputs and its own fp32 scores (for the LeakyReLU slope).  The
    emulation quantises both layers with the first layer's constants."""
    from _quant_stack_grad_ref import quant_stack_grad_f64, within
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    try:
        config.acc, config.fake_quantization, config.w_qbits, config.compute_attention = 0, 1, bits, gat
        config.hardware_quantize, config.float_type = 0, np.float32
        sgrace.init_SGRACE()
        qc = sgrace.quant_constants
        b = _mutag12()
        torch.manual_seed(3)
        model = sgrace.GAT_POOL_PYNQ(7, 16, 2)
        model.eval()                                                        # (dropout off; gradients on)
        kept = {}
        model.reluh.register_forward_hook(lambda m, i, o: kept.__setitem__("D0", o.detach()))
        model.att2.register_forward_hook(lambda m, i, o: kept.__setitem__("D1", o.detach()))
        out = model(b.x, b.edge_index, b.batch)
        out.sum().backward()
        n_graphs = int(b.batch.max()) + 1
        gp = np.ones((n_graphs, 2)) @ model.lin.weight.detach().double().numpy()      # d sum(lin(pooled)) / d pooled
        ei, norm = sgrace.sym_norm2(b.edge_index, b.x.size(0))
        N = b.x.size(0)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0].numpy(), minlength=N))])
        adj = (rowptr, ei[1].numpy(), norm.double().numpy())
        ptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy()))])
        layers = (model.att1, model.att2)
        ws = [c.weight.detach().double().numpy() for c in layers]
        atts = [c.attention.detach().double().numpy().reshape(-1) if gat else None for c in layers]
        outs = [kept["D0"].double().numpy(), kept["D1"].double().numpy()]
        # the emulation's own fp32 scores on the stored entries (FPYNQ_GAT.forward's lines)
        E_dev = [None, None]
        if gat:
            with torch.no_grad():
                X = b.x.float()
                for l, c in enumerate(layers):
                    iq = qc.internal_quantization
                    Wh = torch.mm(sgrace._fq_unsigned(X, qc.f_s, qc.f_z, bits), sgrace._fq_signed(c.weight, qc.w_s, qc.w_z, bits))
                    Wh = torch.round(torch.clip(Wh / (2 ** qc.scale_fea), min=-(2 ** iq - 1) / (2 ** iq), max=(2 ** iq - 1) / (2 ** iq)),
                                     decimals=iq - 1)
                    a = sgrace._fq_signed(c.attention, qc.w_s, qc.w_z, bits)
                    F = c.weight.shape[1]
                    e = c.leakyrelu(torch.matmul(Wh, a[:F, :]) + torch.matmul(Wh, a[F:, :]).T)
                    E_dev[l] = e[ei[0], ei[1]].double().numpy()
                    X = kept["D0"]
        r = quant_stack_grad_f64(adj, b.x.double().numpy(), ws, atts, [True, False], ptr, gp, outs, [qc, qc],
                                 alpha=model.att1.alpha, E_dev=E_dev)
        for l, c in enumerate(layers):
            ok, ratio = within(c.weight.grad.double().numpy(), r["dW"][l], r["mW"][l], r["tW"][l])
            assert ok, (l, "dW", ratio)
            if gat:
                assert r["magnitude"][l] < Q.EXACT_BELOW
                ok, ratio = within(c.attention.grad.double().numpy().reshape(-1), r["dA"][l], r["mA"][l], r["tA"][l])
                assert ok, (l, "dA", ratio)
                assert np.abs(r["dA"][0]).max() > 0
            else:
                assert not c.attention.grad.any()
        assert np.abs(r["dW"][0]).max() > 0
    finally:
        config.restore(saved)
        sgrace.init_SGRACE()


def separating_batch(c, seed, m_in):
    """Ten graphs of 3 to 8 rows, up to four entries a row (the self loop among them): adjacency values over the
    quantiser's range, one neighbour in five stored below half a grid step (it quantises to 0 inside a live row: the
    self loop stays live); features on the feature grid's range [0, 1] and above it."""
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.integers(3, 9, 10)]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    top = (2 ** c.w_qbits - 1) * c.a_s
    rows = []
    for a, n in zip(ptr[:-1], sizes):
        for i in range(n):
            cs = sorted(set(rng.choice(n, min(n, 3), replace=False).tolist()) | {i})
            rows.append([(int(a + k), 0.3 * c.a_s if (k != i and rng.random() < 0.2) else float(rng.uniform(0.6 * c.a_s, top)))
                         for k in cs])
    x = rng.uniform(0.0, 1.3, (int(ptr[-1]), m_in))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return dict(rowptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                col=np.array([k for r in rows for k, _ in r], np.int64), val=f32([v for r in rows for _, v in r]), x=f32(x),
                graph_ptr=ptr, names={}, n_rows=int(ptr[-1]))


def separating_layers(c, m_in, widths, seed):
    """Weights over the signed grid's range and attention vectors that give scores of order 1 on H_q."""
    rng = np.random.default_rng([seed, 9])
    w_max = c.w_s * (1 if c.w_qbits == 1 else 2 ** (c.w_qbits - 1) - 1)
    Ws, atts, m = [], [], m_in
    for P in widths:
        Ws.append(np.asarray(rng.uniform(-1.0, 1.0, (m, P)) * w_max, np.float32).astype(np.float64))
        atts.append(np.asarray(rng.uniform(-1.0, 1.0, 2 * P) * w_max, np.float32).astype(np.float64))
        m = P
    return Ws, atts


@pytest.mark.parametrize("bits", [8, 2])
@pytest.mark.parametrize("mutant", ["scores_unquantised_wh", "d_from_hq", "mask_unquantised"])
def test_mutants_of_the_restatement_leave_the_tolerance(bits, mutant):
    """A backward that took its scores from the unquantised Wh, its d_e from H_q, or its mask from the unquantised
    adjacency lies OUTSIDE the derived tolerance in at least one element of grad_attention or dW -- so the GPU test's
    bound tells the rule from its three nearest mistakes."""
    from _quant_stack_grad_ref import quant_stack_grad_f64
    from sgracex1_amd import quant
    c = quant.constants(bits)
    b = separating_batch(c, 1, 7)
    Ws, atts = separating_layers(c, 7, (20, 7), 3)
    aq = Q.quantise_adj(b["val"], c)
    live_row = np.add.reduceat((aq > 0).astype(int), b["rowptr"][:-1]) > 0
    killed = (aq == 0) & (b["val"] > 0)
    assert killed.any() and live_row.all()                                   # entries that quantise to 0, in live rows
    rng = np.random.default_rng(5)
    gp = rng.standard_normal((len(b["graph_ptr"]) - 1, 7))
    adj = (b["rowptr"], b["col"], b["val"])
    # the forward's D_l by the chain of the quantised forward's restatement (the ReLU mask and X_1).  No ReLU on the top
    # layer: at 2 bits D_0 * deq_o stays below half a step of layer 1's feature grid, so D_1 is 0 and would mask everything
    relus = [True, False]
    import _quant_stack_ref as QS
    ch = QS.chain((b["rowptr"], b["col"]), b["val"], b["x"].astype(np.float32), [W.astype(np.float32) for W in Ws],
                  [a.astype(np.float32) for a in atts], relus, b["graph_ptr"], [c, c])
    outs = [D.astype(np.float64) for D in ch["outs"]]
    assert (outs[0] != 0).any() and (outs[0] == 0).any()                     # layer 0's ReLU mask makes g_0 vary within a graph
    args = (adj, b["x"], Ws, atts, relus, b["graph_ptr"], gp, outs, [c, c])
    ref = quant_stack_grad_f64(*args)
    bad = quant_stack_grad_f64(*args, mutant=mutant)
    outside = False
    for l in range(2):
        for key, m, t in (("dA", "mA", "tA"), ("dW", "mW", "tW")):
            bound = ref[t][l] * ref[m][l] + 1e-30
            outside = outside or bool((np.abs(bad[key][l] - ref[key][l]) > bound).any())
    assert outside, mutant
