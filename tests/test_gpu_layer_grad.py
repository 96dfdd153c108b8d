"""The full layer backward on the kernels against the float64 restatement of the reference's backward
(tests/_layer_grad_ref.py): GATConv_SGRACE (FPYNQ_GAT, config.acc = 1) in GAT and GCN mode, sparse and dense features,
fp32 and fp16 storage, quantised and not; molecule_gcn's FPYNQ + RPYNQ; one NeighborLoader batch through GAT_PYNQ.
Every element of x.grad, weight.grad and attention.grad within TOL of its magnitude bound.  The graphs carry what
the backward treats specially: masked entries (values <= 0), dead rows -- rows the forward gives a uniform softmax over
all N columns, unquantised or only after quantisation -- hub rows past the edge pass's whole-workgroup cut (kRowLong,
256 entries) and the plan's split, rows without entries and an entry count that is not a multiple of 256."""
import numpy as np
import pytest
import torch

import _layer_grad_ref as R
from _fixtures import load

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
# error / magnitude bound.  fp32 sums stay below ~4e-7 of the bound for grad_input / grad_weights and ~2e-9 for
# grad_attention, whose bound is far looser: on a live row the softmax backward's entries sum to 0, so the row sums
# that feed it cancel while their bound adds magnitudes.  A wrong row sum or P^T for P lands at 6e-7 .. 0.6.
TOL = dict(grad_input=1e-5, grad_weights=1e-5, grad_attention=1e-7)
DENSE_MAX = 4096             # the N x N form of the restatement up to here, the edge-list form beyond


def _graph(kind):
    """-> (Csr fp32 on the GPU, features it must show)"""
    from sgracex1_amd import graphs, ops
    if kind == "cora":
        d = load("cora")
        rp, ci, va = d["adj"]
        A = graphs.csr_from_numpy(rp, ci, va, d["N"], dtype=torch.float32)
    elif kind == "masked":
        rowptr, col, val, rows = R.masked_graph(1500, 11, density=0.012)
        A = ops.Csr(rowptr.to(torch.int32).to(dev), col.to(torch.int32).to(dev), val.to(dev), 1500)
    else:                                                           # power law, no self loops: rows without entries
        A = graphs.rmat_graph_n(30_011, 900_000, seed=3, self_loops=False, dtype=torch.float32)
        val = A.val.clone()
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        val[torch.rand(A.nnz, generator=g, device=dev) < 0.01] = -0.5          # stored, masked out
        A = ops.Csr(A.rowptr, A.col, val, A.n_cols)
    deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
    if kind == "rmat":
        assert int(deg.max()) > 2048 and int((deg > 256).sum()) > 10 and int((deg == 0).sum()) > 0 and A.nnz % 256 != 0
        assert A.plan.long_rows > 0                                 # hub rows the aggregation's plan splits
    if kind in ("masked", "rmat"):
        assert bool((A.val <= 0).any()) and bool(R.dead_rows_of(A.rowptr, A.val).any())
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


def _set(gat, dtype, bits, hw):
    from sgracex1_amd import config, sgrace
    config.acc, config.compute_attention, config.device = 1, gat, "cuda"
    config.float_type = np.float16 if dtype == torch.float16 else np.float32
    config.fake_quantization, config.hardware_quantize = int(bits is not None), int(hw)
    config.w_qbits = 32 if bits is None else bits
    sgrace.init_SGRACE()


def _restate(layer, x, W, att, G, gat, gemm, dtype, qc, hw, layer_out, relu, form=None):
    """The layer's own forward quantities (E, S, dead rows), checked, and the restatement's gradients for it."""
    from sgracex1_amd import ops, sgrace
    A = layer._csr
    n = A.n_rows
    dead = None
    if gat:
        fea = (ops.cached_on(x, ("fea_csr", dtype), lambda: None) if gemm == 0 else x.detach().to(dtype).contiguous())
        out, E, S = ops.layer_forward(A, fea, W.t().to(dtype).contiguous(), relu=relu, alpha=layer.alpha,
                                      gat_attention=att.to(dtype).reshape(-1).contiguous(), want_edge_outputs=True,
                                      quant=qc, quant_int8="auto" if (qc is not None and hw) else False)
        assert torch.equal(out.float(), layer_out)                  # the same forward the module ran
        masked = A.val.float() if qc is None else sgrace._fq_unsigned(A.val.float(), qc.a_s, qc.a_z, qc.w_qbits)
        dead = R.dead_rows_of(A.rowptr, masked)
        deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
        row = torch.repeat_interleave(torch.arange(n, device=dev), deg, output_size=A.nnz)
        # the forward's dead rows: a uniform softmax (1 / N on every stored entry), or no entry at all
        uniform = torch.ones(n, dtype=torch.int64, device=dev).index_add_(
            0, row, (~torch.isclose(S, torch.full_like(S, 1.0 / n), rtol=1e-6, atol=0)).long()) == 1
        assert torch.equal(uniform, dead)
        assert not S[(masked[:A.nnz] <= 0) & ~dead[row]].any()       # masked entries of live rows carry no weight
    else:
        E = S = None
    form = form or (R.dense if n <= DENSE_MAX else R.edges)
    return form(A.rowptr, A.col, A.val, x.detach(), W, G, gat=bool(gat), E=E, S=S, dead=dead, alpha=layer.alpha), dead


def _layer_case(kind, gat, gemm, dtype, bits, hw, M, P, seed=0):
    from sgracex1_amd import config, sgrace
    A = _cached_graph(kind)
    n = A.n_rows
    X, W, att, G = _inputs(n, M, P, seed + 31 * P + M, sparse=gemm == 0)
    old = config.snapshot()
    try:
        _set(gat, dtype, bits, hw)
        qc = sgrace.quant_constants
        layer = sgrace.GATConv_SGRACE(M, P).to(dev)
        with torch.no_grad():
            layer.weight.copy_(W), layer.attention.copy_(att)
        x = X.clone().requires_grad_(True)
        relu = 1 if gemm == 0 else 0
        out = layer(gat, gemm, relu, x, None, A.val, A)
        out.backward(G)
        (grads, bounds), dead = _restate(layer, x, W, att, G, gat, gemm, dtype, qc, hw, out.detach(), relu)
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
    got = dict(grad_input=x.grad, grad_weights=layer.weight.grad)
    if gat:
        got["grad_attention"] = layer.attention.grad
    else:
        assert not layer.attention.grad.any()
    figures = R.check(got, grads, bounds, TOL, (kind, gat, gemm, dtype, bits, hw, M, P))
    print("layer_grad", kind, gat, gemm, dtype, bits, hw, M, P, "dead", int(dead.sum()) if dead is not None else 0,
          {k: f"{v:.2e}" for k, v in figures.items()})
    return dead


@pytest.mark.parametrize("P", [7, 16, 64, 300])
@pytest.mark.parametrize("M", [7, 602])
@pytest.mark.parametrize("gemm", [0, 1])
def test_layer_grad_widths_on_the_masked_graph(gemm, M, P):
    """GAT, fp32 and fp16 storage: every width of the padded Wh path and of xw_dense's pad columns, on a graph with
    masked entries and dead rows."""
    for dtype in (torch.float32, torch.float16):
        dead = _layer_case("masked", 1, gemm, dtype, None, 0, M, P)
        assert int(dead.sum()) >= 2


@pytest.mark.parametrize("bits,hw", [(None, 0), (8, 0), (8, 1), (4, 0), (1, 0)])
@pytest.mark.parametrize("gat,gemm", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_layer_grad_quantised_on_the_masked_graph(gat, gemm, bits, hw):
    """Both modes and feature forms, quantiser off, 8 bits (emulated grid and the int8 matrix cores), 4 and 1 bits:
    quantised, the forward's dead rows are those of the QUANTISED adjacency, the backward masks with the unquantised."""
    dead = _layer_case("masked", gat, gemm, torch.float32, bits, hw, 602, 16)
    if gat:
        assert int(dead.sum()) >= (2 if bits is None else 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("gat,gemm", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_layer_grad_cora(gat, gemm, dtype):
    _layer_case("cora", gat, gemm, dtype, None, 0, 602, 16)


@pytest.mark.parametrize("gat,gemm,dtype,bits,hw,M,P", [
    (1, 1, torch.float32, None, 0, 7, 64),
    (1, 0, torch.float16, None, 0, 602, 16),
    (1, 1, torch.float16, None, 0, 7, 300),
    (0, 1, torch.float32, None, 0, 7, 16),
    (1, 1, torch.float32, 4, 0, 7, 16),
    (1, 1, torch.float32, 8, 1, 602, 7),
])
def test_layer_grad_power_law(gat, gemm, dtype, bits, hw, M, P):
    """30 K nodes (edge-list restatement): hub rows, rows without entries, masked entries; at 4 bits most rows of a
    power-law graph quantise to all-zero and so are dead in the forward while their entries stay live in the mask."""
    dead = _layer_case("rmat", gat, gemm, dtype, bits, hw, M, P)
    if bits == 4:
        assert int(dead.sum()) > 100


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("P", [2, 7, 64])
@pytest.mark.parametrize("M,plan", [(7, True), (602, False)])
def test_fpynq_layer_grad_power_law(M, plan, P, relu):
    """molecule_gcn.GraphConvolution_pynq (FPYNQ, sparse X, fp16 storage) followed by RPYNQ: grad_W = X^T A g and
    grad_x = A g W^T with g masked where the layer's output is exactly 0.  X^T of 7 rows and 30 K entries gets a plan
    (the MUTAG shape), X^T of 602 rows and a few thousand entries does not."""
    from sgracex1_amd import molecule_gcn as MG, pynq_shim
    A = _cached_graph("rmat")
    n = A.n_rows
    g = torch.Generator(device=dev)
    g.manual_seed(M + P)
    if M == 7:                                                      # one-hot node labels, as MUTAG's
        X = torch.nn.functional.one_hot(torch.randint(0, M, (n,), generator=g, device=dev), M).float()
    else:
        X = torch.zeros((n, M), device=dev)
        X.view(-1)[torch.randint(0, n * M, (4000,), generator=g, device=dev)] = torch.rand(4000, generator=g, device=dev)
        X = X.half().float()
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    layer = MG.GraphConvolution_pynq(M, P, ip).to(dev)
    with torch.no_grad():
        layer.weight.copy_(layer.weight.half().float())
    x = X.clone().requires_grad_(True)
    out = layer(1, 0, relu, x, A)
    y = MG.Relu_pynq()(out)
    G = torch.randn(y.shape, generator=g, device=dev).to(y.dtype)
    y.backward(G)
    assert (out == 0).any() and (out != 0).any()
    Xt = MG.feature_csr(x, MG.ACC_DTYPE)._transposed
    assert (Xt._plan is not None) == plan and (Xt.nnz >= 64 * Xt.n_rows) == plan
    Gl = G.float() * (out.detach() != 0)                            # RPYNQ: the gradient where the output is not 0
    Af = A.to(MG.ACC_DTYPE)                                         # the adjacency the layer stored
    grads, bounds = R.edges(Af.rowptr, Af.col, Af.val, X, layer.weight.detach(), Gl)
    figures = R.check(dict(grad_input=x.grad, grad_weights=layer.weight.grad), grads, bounds, TOL, (M, P, relu))
    print("fpynq_grad", M, P, relu, {k: f"{v:.2e}" for k, v in figures.items()})


@pytest.mark.parametrize("out_dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("grad_dtype", [torch.float16, torch.float32])
def test_rpynq_masks_zero_and_negative_zero(out_dtype, grad_dtype):
    """RPYNQ.backward (relu_mask_backward_): the gradient is 0 exactly where the layer output is +0.0 or -0.0, and kept
    bit for bit elsewhere, for every pairing of output and gradient element types."""
    from sgracex1_amd import molecule_gcn as MG
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    out = torch.randn((1001, 7), generator=g, device=dev)
    out[torch.rand(out.shape, generator=g, device=dev) < 0.2] = 0.0
    out[torch.rand(out.shape, generator=g, device=dev) < 0.2] = -0.0
    out = out.to(out_dtype)
    assert bool((out == 0).any()) and bool(torch.signbit(out[out == 0]).any()) and bool((~torch.signbit(out[out == 0])).any())
    G = torch.randn((1001, 7), generator=g, device=dev).to(grad_dtype)

    class ctx:
        saved_tensors = (out,)
    gx = MG.RPYNQ.backward(ctx, G)
    want = torch.where(out == 0, torch.zeros_like(G), G)
    assert gx.dtype == G.dtype and torch.equal(gx, want.to(gx.dtype))


@pytest.mark.parametrize("bits", [None, 4])
def test_layer_grad_neighbor_loader_batch(bits):
    """One NeighborLoader batch (fan-outs [10, 5]) of cora through GAT_PYNQ, fp32 and 4 bits: both layers' gradients
    against the restatement on the batch's subgraph, fed each layer's input and the gradient that reached its output."""
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
    loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(X, ei), [10, 5], batch_size=64, seed=2)
    batch = next(iter(loader))
    old = config.snapshot()
    seen = {}
    try:
        _set(1, torch.float32, bits, 0)
        qc = sgrace.quant_constants
        torch.manual_seed(4)
        model = sgrace.GAT_PYNQ(d["M_fea"], 16, 1, 7).to(dev).eval()

        def hook(mod, args, out):
            seen[mod] = dict(x=args[3], relu=args[2], gemm=args[1], out=out.detach())
            out.register_hook(lambda g: seen[mod].__setitem__("g", g.clone()))

        for layer in (model.att2, model.conv22):
            layer.register_forward_hook(hook)
        x = batch.x.clone().requires_grad_(True)
        logits = model(x, batch.edge_index)
        torch.nn.functional.cross_entropy(logits[:batch.batch_size], torch.arange(batch.batch_size, device=dev) % 7).backward()
        for k, layer in enumerate((model.att2, model.conv22)):
            s = seen[layer]
            lq = None if qc is None else (qc if k == 0 else qc.second_layer())
            (grads, bounds), dead = _restate(layer, s["x"], layer.weight.detach(), layer.attention.detach(), s["g"], 1,
                                             s["gemm"], torch.float32, lq, 0, s["out"], s["relu"], form=R.edges)
            got = dict(grad_weights=layer.weight.grad, grad_attention=layer.attention.grad)
            if k == 0:                                  # (layer 2's grad_input went on through RPYNQ into layer 1's g)
                got["grad_input"] = x.grad
            figures = R.check(got, grads, bounds, TOL, ("batch", bits, k))
            print("batch_grad", bits, k, "dead", int(dead.sum()), {kk: f"{v:.2e}" for kk, v in figures.items()})
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
