"""The layer backward as one C ABI call (config.accb = 1, sgx_layer_backward) against the float64 restatement of the
reference's backward (tests/_layer_grad_ref.py) and against the composed path (config.accb = 0), and its new stage
sgx_gat_attention_grad on its own.  Tolerances are those of test_gpu_layer_grad.py: error / magnitude bound, where the
fp32 path sits near 4e-7 (grad_input, grad_weights) and 2e-9 (grad_attention) and a wrong row sum or P^T lands at 6e-7 or
above."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _layer_grad_ref as R
from _fixtures import load

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(grad_input=1e-5, grad_weights=1e-5, grad_attention=1e-7)
DENSE_MAX = 4096


def _graph(kind):
    from sgracex1_amd import graphs, ops
    if kind == "masked":
        rowptr, col, val, rows = R.masked_graph(1500, 11, density=0.012)
        A = ops.Csr(rowptr.to(torch.int32).to(dev), col.to(torch.int32).to(dev), val.to(dev), 1500)
        assert bool((A.val <= 0).any()) and int(R.dead_rows_of(A.rowptr, A.val).sum()) >= 2
        deg = A.rowptr[1:] - A.rowptr[:-1]
        assert int(deg[rows["empty"]]) == 0
        return A
    if kind == "wide":
        # 70 001 rows of which only the first 100 hold an entry (a self loop): every other row is dead, and at 256 columns
        # the elements of the dead rows from row 65 536 on lie past 2^24 -- beyond one pass of any launch capped at 65 536
        # workgroups of 256 threads
        n = 70_001
        rowptr = torch.cat([torch.arange(101), torch.full((n - 100,), 100)]).to(torch.int32).to(dev)
        A = ops.Csr(rowptr, torch.arange(100, dtype=torch.int32, device=dev), torch.ones(100, device=dev), n)
        assert int(R.dead_rows_of(A.rowptr, A.val).sum()) == n - 100 and (n - 1) * 256 > 2 ** 24
        return A
    # power law, no self loops: hub rows, rows without entries; 1 % of the entries stored and masked out
    A = graphs.rmat_graph_n(30_011, 900_000, seed=3, self_loops=False, dtype=torch.float32)
    val = A.val.clone()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    val[torch.rand(A.nnz, generator=g, device=dev) < 0.01] = -0.5
    A = ops.Csr(A.rowptr, A.col, val, A.n_cols)
    deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
    assert int(deg.max()) > 2048 and int((deg > 256).sum()) > 10 and int((deg == 0).sum()) > 0 and A.nnz % 256 != 0
    return A


_GRAPHS = {}


def _cached_graph(kind):
    if kind not in _GRAPHS:
        _GRAPHS[kind] = _graph(kind)
    return _GRAPHS[kind]


def _inputs(n, M, P, seed, sparse):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    X = torch.rand((n, M), generator=g, device=dev)
    X = X * (torch.rand((n, M), generator=g, device=dev) < (0.05 if sparse else 0.6))
    X = X.half().float()                                            # the same values in fp16 and fp32 storage
    W = ((torch.rand((M, P), generator=g, device=dev) * 2 - 1) * (1.5 / M ** 0.5)).half().float()
    att = ((torch.rand((2 * P, 1), generator=g, device=dev) * 2 - 1) * 0.7).half().float()
    G = torch.randn((n, P), generator=g, device=dev)
    return X, W, att, G


def _set(gat, dtype, bits, accb, lean):
    from sgracex1_amd import config, sgrace
    config.acc, config.accb, config.compute_attention, config.device = 1, accb, gat, "cuda"
    config.gat_edge_outputs = 0 if lean else 1
    config.float_type = np.float16 if dtype == torch.float16 else np.float32
    config.fake_quantization, config.hardware_quantize = int(bits is not None), 0
    config.w_qbits = 32 if bits is None else bits
    sgrace.init_SGRACE()


def _restate(layer, x, W, att, G, gat, gemm, dtype, qc, layer_out, relu, form=None, lean=False):
    """The forward's own quantities (E, S, dead rows) and the restatement's gradients for them."""
    from sgracex1_amd import ops, sgrace
    A = layer._csr
    dead = E = S = None
    if gat:
        fea = (ops.cached_on(x, ("fea_csr", dtype), lambda: None) if gemm == 0 else x.detach().to(dtype).contiguous())
        out, E, S = ops.layer_forward(A, fea, W.t().to(dtype).contiguous(), relu=relu, alpha=layer.alpha,
                                      gat_attention=att.to(dtype).reshape(-1).contiguous(), want_edge_outputs=True, quant=qc)
        if lean:            # (the forward without side outputs may take the one walk, whose D differs in the last bits)
            assert torch.allclose(out.float(), layer_out, rtol=1e-3, atol=1e-4)
        else:
            assert torch.equal(out.float(), layer_out)              # the same forward the module ran
        masked = A.val.float() if qc is None else sgrace._fq_unsigned(A.val.float(), qc.a_s, qc.a_z, qc.w_qbits)
        dead = R.dead_rows_of(A.rowptr, masked)
    form = form or (R.dense if A.n_rows <= DENSE_MAX else R.edges)
    return form(A.rowptr, A.col, A.val, x.detach(), W, G, gat=bool(gat), E=E, S=S, dead=dead, alpha=layer.alpha), dead


def _run_layer(kind, gat, gemm, dtype, bits, M, P, accb, lean=False, x_grad=True, seed=0, restate=True):
    """One GATConv_SGRACE forward + backward -> (gradients, (grads, bounds) of the restatement or None, dead rows)."""
    from sgracex1_amd import config, sgrace
    A = _cached_graph(kind)
    X, W, att, G = _inputs(A.n_rows, M, P, seed + 31 * P + M, sparse=gemm == 0)
    old = config.snapshot()
    ref = dead = None
    try:
        _set(gat, dtype, bits, accb, lean)
        qc = sgrace.quant_constants
        layer = sgrace.GATConv_SGRACE(M, P).to(dev)
        with torch.no_grad():
            layer.weight.copy_(W), layer.attention.copy_(att)
        x = X.clone().requires_grad_(x_grad)
        relu = 1 if gemm == 0 else 0
        out = layer(gat, gemm, relu, x, None, A.val, A)
        out.backward(G)
        if restate:
            ref, dead = _restate(layer, x, W, att, G, gat, gemm, dtype, qc, out.detach(), relu, lean=lean)
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
    got = dict(grad_weights=layer.weight.grad)
    if x_grad:
        got["grad_input"] = x.grad
    else:
        assert x.grad is None
    if gat:
        got["grad_attention"] = layer.attention.grad
    else:
        assert not layer.attention.grad.any()
    return got, ref, dead


def _check(got, ref, what):
    figures = R.check(got, ref[0], ref[1], TOL, what)
    print("layer_backward", *what, {k: f"{v:.2e}" for k, v in figures.items()})
    return figures


# ---- 1. the call against float64 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("M,P", [(7, 7), (7, 64), (602, 16), (602, 300)])
@pytest.mark.parametrize("gemm", [0, 1])
@pytest.mark.parametrize("gat,lean", [(1, False), (1, True), (0, False)])
def test_one_call_against_float64(gat, lean, gemm, M, P):
    """GAT (E, S and statistics forms) and GCN, CSR and dense features, fp32 and fp16 adjacency storage, odd widths,
    sub-dword fp16 rows, P > 256 and K > 128, on the graph with masked entries, an empty row and dead rows."""
    for dtype in (torch.float32, torch.float16):
        got, ref, dead = _run_layer("masked", gat, gemm, dtype, None, M, P, accb=1, lean=lean)
        _check(got, ref, ("masked", gat, lean, gemm, dtype, M, P))
        if gat:
            assert int(dead.sum()) >= 2


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("lean", [False, True])
def test_one_call_quantised(bits, lean):
    """Quantised, the forward's dead rows are those of the quantised adjacency while the mask stays the unquantised one."""
    got, ref, dead = _run_layer("masked", 1, 1, torch.float32, bits, 602, 16, accb=1, lean=lean)
    _check(got, ref, ("masked", "bits", bits, lean))
    assert int(dead.sum()) >= 3


# ---- 2. hub rows -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [16, 64])
def test_one_call_hub_rows(P):
    """30 K nodes of a power-law graph (edge-list restatement): rows over 2048 and over 256 entries go through the
    attention gradient's chunked walk, rows without entries through its empty chain."""
    got, ref, dead = _run_layer("rmat", 1, 1, torch.float32, None, 7, P, accb=1)
    _check(got, ref, ("rmat", P))
    assert int(dead.sum()) > 0


def test_one_call_dead_rows_past_2_to_24_elements(gat=1):
    """Dead rows whose elements of P . G lie past index 2^24 (row 65 536 and up at 256 columns) get colsum(G) / N like
    every other dead row: all of grad_input is checked, and grad_weights sums over every row."""
    got, ref, dead = _run_layer("wide", gat, 1, torch.float32, None, 7, 256, accb=1)
    _check(got, ref, ("wide", gat))
    assert bool(dead[65_536:].all())
    row = got["grad_input"][70_000]
    assert bool(row.any()) and torch.equal(row, got["grad_input"][200])            # one and the same uniform row of P


# ---- 3. the attention gradient alone ---------------------------------------------------------------------------------

def _random_csr(n_rows, n_cols, degs, seed):
    from sgracex1_amd import ops
    g = torch.Generator().manual_seed(seed)
    degs = torch.as_tensor(degs, dtype=torch.int64)
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(degs, 0)
    col = torch.randint(0, n_cols, (int(rowptr[-1]),), generator=g)
    return ops.Csr(rowptr.to(torch.int32).to(dev), col.to(torch.int32).to(dev),
                   torch.ones(int(rowptr[-1]), dtype=torch.float32, device=dev), n_cols)


def _attention_grad_case(n_rows, n_cols, P, degs, seed, padded):
    from sgracex1_amd import ops
    A = _random_csr(n_rows, n_cols, degs, seed)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nnz = A.nnz
    sg = torch.randn(nnz, generator=g, device=dev) if nnz else torch.zeros(1, device=dev)
    row = R._rows(A.rowptr.long(), nnz)
    g1 = torch.zeros(n_rows, device=dev).index_add_(0, row, sg[:nnz]) if nnz else torch.zeros(n_rows, device=dev)
    if nnz:
        g1 = g1 + 0.25 * torch.randn(n_rows, generator=g, device=dev)              # any g1, not only the row sums
    pitch = ops.table_pitch(P, 4) if padded else P
    Wh = torch.randn((n_cols, pitch), generator=g, device=dev)[:, :P]
    return attention_grad_check(A, sg, g1, Wh, (n_rows, n_cols, P, "nnz", nnz, "padded", padded))


def attention_grad_check(A, sg, g1, Wh, what):
    """ops.gat_attention_grad on these operands: the same bits twice, and within TOL of float64 Wh^T g1 and Wh^T colsum(sg)
    by the bounds |Wh|^T |g1| and |Wh|^T colsum|sg|."""
    from sgracex1_amd import ops
    n_rows, n_cols, nnz = A.n_rows, A.n_cols, A.nnz
    out = ops.gat_attention_grad(A, sg, g1, Wh)
    again = ops.gat_attention_grad(A, sg, g1, Wh)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))              # the same bits on every run
    Wd, sd = Wh.double(), sg[:nnz].double()
    col = A.col[:nnz].long()
    cs = torch.zeros(n_cols, dtype=torch.float64, device=dev).index_add_(0, col, sd)
    cs_abs = torch.zeros(n_cols, dtype=torch.float64, device=dev).index_add_(0, col, sd.abs())
    want = torch.cat([Wd[:n_rows].t() @ g1.double(), Wd.t() @ cs])
    bound = torch.cat([Wd[:n_rows].abs().t() @ g1.double().abs(), Wd.abs().t() @ cs_abs])
    ratio = R.worst(out, want, bound)
    print("attention_grad", *what, f"{ratio:.2e}")
    assert torch.isfinite(out).all() and ratio <= TOL["grad_attention"], ratio
    return out


@pytest.mark.parametrize("P", [1, 7, 16, 300])
@pytest.mark.parametrize("padded", [True, False])
def test_attention_grad_alone(P, padded):
    """Against float64 Wh^T g1 and Wh^T colsum(sg), bound |Wh|^T |g1| and |Wh|^T colsum|sg|: one row; 1000 rows (not a
    multiple of the 63 rows a workgroup takes, nor of its lane groups) with empty rows, rows of exactly 256 and 257
    entries and a row of 5000 (more chunks than a workgroup has lane groups at P = 300); the padded pitch (16-byte
    gathers) and the plain one (element gathers)."""
    _attention_grad_case(1, 5, P, [3], 1, padded)
    rng = np.random.default_rng(5)
    degs = rng.integers(0, 40, 1000)
    degs[[0, 7, 500]] = 0
    degs[11], degs[12], degs[640], degs[999] = 256, 257, 5000, 300
    _attention_grad_case(1000, 1200, P, degs, 2, padded)


@pytest.mark.parametrize("P", [1, 7, 300])
def test_attention_grad_without_entries(P):
    out = _attention_grad_case(130, 130, P, [0] * 130, 3, True)
    assert not out.any()                                                            # both halves exactly 0


# ---- 4. same kernels, same bits --------------------------------------------------------------------------------------

@pytest.mark.parametrize("gat,gemm", [(0, 1), (1, 1), (0, 0), (1, 0)])
def test_one_call_against_the_composed_path(gat, gemm):
    """accb = 1 runs the products on the stage kernels of accb = 0 with the same arguments: dense features give the same
    bits for grad_input and grad_weights (GCN, and GAT from E and S, on a graph with dead rows); CSR features sum
    grad_weights in another order (the CSR of X^T instead of the dense X), so they stay within tolerance; grad_attention
    is formed by another kernel and stays within tolerance of the restatement and of the accb = 0 value."""
    one, ref, dead = _run_layer("masked", gat, gemm, torch.float32, None, 602, 16, accb=1)
    two, _, _ = _run_layer("masked", gat, gemm, torch.float32, None, 602, 16, accb=0, restate=False)
    _check(one, ref, ("masked", "accb 1", gat, gemm))
    _check(two, ref, ("masked", "accb 0", gat, gemm))
    if gemm == 1:
        assert torch.equal(one["grad_input"], two["grad_input"])
        assert torch.equal(one["grad_weights"], two["grad_weights"])
    if gat:
        bound = ref[1]["grad_attention"]
        ratio = R.worst(one["grad_attention"], two["grad_attention"].double(), bound)
        print("accb 1 against accb 0, grad_attention", f"{ratio:.2e}")
        assert ratio <= TOL["grad_attention"]


# ---- 5. grad_input is skipped ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("gat,gemm,lean", [(1, 0, False), (1, 1, True), (0, 1, False)])
def test_grad_input_is_skipped(gat, gemm, lean):
    with_x, _, _ = _run_layer("masked", gat, gemm, torch.float32, None, 602, 16, accb=1, lean=lean, restate=False)
    without, _, _ = _run_layer("masked", gat, gemm, torch.float32, None, 602, 16, accb=1, lean=lean, x_grad=False, restate=False)
    assert "grad_input" in with_x and "grad_input" not in without                  # (x.grad is None: _run_layer)
    for name in without:
        assert torch.equal(with_x[name].view(torch.int32), without[name].view(torch.int32)), name


# ---- 6. the module and the loaders -----------------------------------------------------------------------------------

@pytest.mark.parametrize("gat", [1, 0])
def test_one_call_neighbor_loader_batch(gat):
    """One NeighborLoader(prepare="sym_norm2") batch of cora through GAT_PYNQ with accb = 1: both layers' gradients against
    the restatement on the batch's subgraph; the whole backward runs without a synchronisation."""
    from sgracex1_amd import config, pyg_lite, sgrace
    d = load("cora")
    n = d["N"]
    rp, ci, _ = d["adj"]
    row = np.repeat(np.arange(n), np.diff(rp))
    keep = row != ci
    ei = torch.as_tensor(np.stack([row[keep], ci[keep]]), dtype=torch.int64, device=dev)
    X = torch.zeros((n, d["M_fea"]), device=dev)
    frow = np.repeat(np.arange(n), np.diff(d["fea"][0]))
    X[torch.as_tensor(frow, device=dev), torch.as_tensor(d["fea"][1].astype(np.int64), device=dev)] = 1.0
    loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(X, ei), [10, 5], batch_size=64, seed=2, prepare="sym_norm2")
    batch = next(iter(loader))
    old = config.snapshot()
    seen = {}
    try:
        _set(gat, torch.float32, None, 1, False)
        torch.manual_seed(4)
        model = sgrace.GAT_PYNQ(d["M_fea"], 16, 1, 7).to(dev).eval()

        def hook(mod, args, out):
            seen[mod] = dict(x=args[3], relu=args[2], gemm=args[1], out=out.detach())
            out.register_hook(lambda g: seen[mod].__setitem__("g", g.clone()))

        for layer in (model.att2, model.conv22):
            layer.register_forward_hook(hook)
        x = batch.x.requires_grad_(True)
        logits = model(x, batch.edge_index_agg)
        loss = torch.nn.functional.cross_entropy(logits[:batch.batch_size], torch.arange(batch.batch_size, device=dev) % 7)
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        for k, layer in enumerate((model.att2, model.conv22)):
            s = seen[layer]
            ref, dead = _restate(layer, s["x"], layer.weight.detach(), layer.attention.detach(), s["g"], gat, s["gemm"],
                                 torch.float32, None, s["out"], s["relu"], form=R.edges)
            got = dict(grad_weights=layer.weight.grad)
            if gat:
                got["grad_attention"] = layer.attention.grad
            if k == 0:                                  # (layer 2's grad_input went on through RPYNQ into layer 1's g)
                got["grad_input"] = x.grad
            _check(got, ref, ("batch", gat, k))
    finally:
        config.restore(old)
        sgrace.init_SGRACE()


def test_one_call_is_capturable():
    """sgx_layer_backward neither allocates nor synchronises: the whole call (GAT from E and S, dead rows, grad_input) is
    captured in a graph -- a synchronisation or an allocation inside the library would fail the capture -- and the replay
    gives the bits of the eager call."""
    from sgracex1_amd import ops
    A = _cached_graph("masked")
    M, P = 602, 16
    X, W, att, G = _inputs(A.n_rows, M, P, 5, sparse=False)
    out, E, S = ops.layer_forward(A, X, W.t().contiguous(), gat_attention=att.reshape(-1).contiguous(), want_edge_outputs=True)
    dead = A.dead_rows
    assert A.has_dead_rows
    call = lambda: ops.layer_backward(A, X, W, G, gat=True, gemm_mode=1, E=E, S=S, dead=dead)
    eager = call()                                         # (also builds the adjacency's plan, which is not capturable)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                             # the workspace of this stream, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = call()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("grad_input", "grad_weights", "grad_attention"), eager, captured):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


# ---- 7. the example --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mini", [False, True])
def test_example_trains_with_accb(mini):
    """examples/sgrace_node_classification.py --attention --accb, full graph and device-built mini-batches: the test
    accuracy of the accb = 0 run of the same seed, less the 0.02 a twin is given."""
    from sgracex1_amd import config, sgrace
    spec = importlib.util.spec_from_file_location("sgrace_nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kw = dict(batch_size=128, num_neighbors=[10, 10], device_batches=True) if mini else {}
    old = config.snapshot()
    try:
        acc = {}
        for accb in (0, 1):
            res, _, _ = mod.run(attention=True, acc=1, epochs=40, n=2000, verbose=False, accb=accb, **kw)
            acc[accb] = res["test_acc"]
        print("example", "mini" if mini else "full", acc)
        assert acc[1] >= acc[0] - 0.02
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
