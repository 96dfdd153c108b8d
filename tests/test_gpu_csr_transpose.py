"""sgx_csr_transpose on the GPU: all five outputs of the C ABI call against the numpy restatement of its rule
(tests/_transpose_ref.py), exactly; then ops.csr_transpose(method="device") against method="torch", the NeighborLoader's
transposed=True batches, and the example."""
import ctypes
import importlib.util
import os
import time

import numpy as np
import pytest
import torch

import _transpose_ref as TR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
_TORCH = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32}
_BITS = {torch.float16: torch.int16, torch.float32: torch.int32}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _abi(rowptr, col, val, n_rows, n_cols, nnz, want_order=True):
    """One call on device tensors (any 4- / 2-byte aligned slices) -> (rowptr_t, col_t, val_t or None, order or None)."""
    from sgracex1_amd import _lib
    lib = _lib.lib
    rowptr_t = torch.full((n_cols + 1,), -7, dtype=torch.int32, device=DEV)
    col_t = torch.full((max(nnz, 1),), -7, dtype=torch.int32, device=DEV)
    val_t = None if val is None else torch.zeros(max(nnz, 1), dtype=val.dtype, device=DEV)
    order = torch.full((max(nnz, 1),), -7, dtype=torch.int32, device=DEV) if want_order else None
    need = lib.sgx_csr_transpose_workspace_bytes(n_rows, n_cols, nnz)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    code = 99 if val is None else {torch.float16: _lib.SGX_F16, torch.float32: _lib.SGX_F32}[val.dtype]   # (not looked at without values)
    status = lib.sgx_csr_transpose(code, n_rows, n_cols, nnz, _p(rowptr), _p(col), _p(val), _p(rowptr_t), _p(col_t), _p(val_t),
                                   _p(order), _p(ws), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0, status
    return rowptr_t, col_t[:nnz], None if val is None else val_t[:nnz], None if order is None else order[:nnz]


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int16 if a.dtype == np.float16 else np.int32)


def _check(rowptr, col, val, n_cols, want_order=True):
    """The call on a host CSR against the restatement: every output exactly, values as raw bits."""
    rowptr, col = np.asarray(rowptr, np.int32), np.asarray(col, np.int32)
    n_rows, nnz = len(rowptr) - 1, int(rowptr[-1])
    d_col = _dev(col if nnz else np.zeros(1, np.int32))
    d_val = None if val is None else _dev(val if nnz else np.zeros(1, val.dtype))
    got = _abi(_dev(rowptr), d_col, d_val, n_rows, n_cols, nnz, want_order)
    torch.cuda.synchronize()
    rp_t, col_t, val_t, order = TR.transpose(rowptr, col, val, n_cols)
    assert np.array_equal(got[0].cpu().numpy(), rp_t)
    assert np.array_equal(got[1].cpu().numpy(), col_t)
    if val is not None:
        assert np.array_equal(_bits(got[2].cpu().numpy()), _bits(val_t))
    if want_order:
        assert np.array_equal(got[3].cpu().numpy(), order)
    return got


def _tile():
    from sgracex1_amd import _lib
    return _lib.SGX_CSR_TRANSPOSE_TILE


# ---- 1. degenerate shapes ---------------------------------------------------------------------------------------------

def test_degenerate_shapes():
    rng = np.random.default_rng(0)
    _check([0], [], np.zeros(0, np.float32), 5)                                    # n_rows = 0
    _check([0, 0, 0, 0, 0], [], np.zeros(0, np.float32), 5)                        # nnz = 0, n_cols = 5
    _check([0], [], None, 0)                                                       # nothing at all
    col = rng.permutation(500)[:200].astype(np.int32)
    _check([0, 200], col, rng.standard_normal(200).astype(np.float32), 500)        # one row, columns in no order
    rowptr, _, val = TR.random_csr(rng, 300, 1, 3000)
    _check(rowptr, np.zeros(3000, np.int32), val, 1)                               # n_cols = 1: one transposed row
    rowptr, col, val = TR.random_csr(rng, 60, 200, 2500)
    rowptr = np.concatenate([np.zeros(3, np.int32), rowptr])                       # the first 3 rows empty,
    _check(rowptr, col, val, 500)                                                  # the last 300 columns too


# ---- 2. digit and scan edges ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cols", [2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24 + 1])
def test_column_counts_at_the_digit_edges(n_cols):
    rng = np.random.default_rng(n_cols)
    n_rows, nnz = 700, 5000
    row = np.sort(rng.integers(0, n_rows, nnz))
    col = rng.integers(0, n_cols, nnz)
    col[:40] = 0
    col[-40:] = n_cols - 1                                                         # the first and the last column are used
    col[rng.permutation(nnz)[:200]] = rng.choice([0, n_cols - 1, min(255, n_cols - 1), min(256, n_cols - 1)], 200)
    rowptr = np.zeros(n_rows + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    got = _check(rowptr, col, rng.standard_normal(nnz).astype(np.float32), n_cols)
    assert int(got[0][-1]) == nnz


# ---- 3. tile edges ----------------------------------------------------------------------------------------------------

def test_entry_counts_at_the_tile_edges():
    tile = _tile()
    wave = tile // 4                                       # a wavefront's share of a tile
    for nnz in (1, 63, 64, 65, wave - 1, wave, wave + 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1,
                256 * tile + 1):                           # the last: more tiles than one step of the scan over tiles takes
        rng = np.random.default_rng(nnz)
        for n_cols in (37, 1000):                          # one pass, two passes
            rowptr, col, val = TR.random_csr(rng, 91, n_cols, nnz)
            _check(rowptr, col, val, n_cols)


# ---- 4. stability -----------------------------------------------------------------------------------------------------

def test_repeated_pairs_keep_their_source_order():
    rng = np.random.default_rng(7)
    n_rows, n_cols, nnz = 400, 300, 20000
    first = int(nnz * 0.6)
    flat = rng.choice(n_rows * n_cols, size=first, replace=False)
    flat = np.concatenate([flat, rng.choice(flat, size=nnz - first)])              # 40 % repeat an earlier (row, col)
    flat = flat[rng.permutation(nnz)]
    flat = flat[np.argsort(flat // n_cols, kind="stable")]                         # by row only: columns in no order
    row, col = flat // n_cols, flat % n_cols
    rowptr = np.zeros(n_rows + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    val = np.arange(nnz, dtype=np.float32)                                         # every copy its own value
    assert len(np.unique(flat)) <= first
    _check(rowptr, col, val, n_cols)


def test_one_long_transposed_row_is_linear_work():
    """A column of 300 000 entries among 64 sparse ones: a transposed row across ~150 tiles.  Linear work on 300 K entries is
    well under a millisecond of kernels; a step quadratic in the row (L^2 / 256 lane steps measured 351 ms at L = 70 000) would take
    seconds.  The bound is half a second of wall clock for the call and its synchronisation, after a warm-up on a small
    matrix."""
    rng = np.random.default_rng(3)
    n_rows, n_cols = 300000, 65
    extra_rows = np.sort(rng.integers(0, n_rows, 2000))
    extra_cols = rng.choice(np.delete(np.arange(n_cols), 32), 2000)
    row = np.concatenate([np.arange(n_rows), extra_rows])
    col = np.concatenate([np.full(n_rows, 32), extra_cols])
    o = np.lexsort((col, row))
    row, col = row[o], col[o].astype(np.int32)
    rowptr = np.zeros(n_rows + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    val = rng.standard_normal(len(col)).astype(np.float32)
    _check(*TR.random_csr(rng, 50, 65, 3000), 65)                                  # warm-up: code objects, first launches
    d = _dev(rowptr), _dev(col), _dev(val)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _abi(*d, n_rows, n_cols, len(col))
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    print(f"300 000-entry column: {took * 1e3:.2f} ms")
    got = _check(rowptr, col, val, n_cols)
    assert int(got[0][33] - got[0][32]) >= 300000
    assert took < 0.5, took


# ---- 5. values --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_values_are_copied_bit_for_bit(dtype):
    rng = np.random.default_rng(11)
    rowptr, col, val = TR.random_csr(rng, 200, 300, 6000, dtype=dtype)
    bits = _bits(val)
    info = np.finfo(dtype)
    special = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, info.smallest_subnormal, -info.smallest_subnormal,
                        info.tiny / 2, info.max, info.tiny], dtype=dtype)
    val[:len(special)] = special
    # NaN payloads, quiet and signalling, both signs; the largest subnormal
    payloads = [0x7E01, 0x7D55, 0xFE01, 0xFC01, 0x03FF] if dtype == np.float16 else \
        [0x7FC00001, 0x7FA55555, 0xFFC12345, 0xFF800001, 0x007FFFFF]
    bits[20:25] = np.array(payloads, dtype=np.uint32).astype(np.uint16 if dtype == np.float16 else np.uint32).view(bits.dtype)
    val[100 + rng.permutation(len(val) - 100)[:50]] = -0.0
    _check(rowptr, col, val, 300)


def test_pattern_only_and_without_order():
    rng = np.random.default_rng(12)
    rowptr, col, val = TR.random_csr(rng, 150, 700, 5000)
    _check(rowptr, col, None, 700)                         # values = NULL (and a dtype code that is no type)
    _check(rowptr, col, val, 700, want_order=False)        # order = NULL
    _check(rowptr, col, None, 700, want_order=False)


def test_inputs_as_slices_at_odd_element_offsets():
    rng = np.random.default_rng(13)
    rowptr, col, val = TR.random_csr(rng, 150, 700, 5001, dtype=np.float16)
    n_rows, nnz = 150, int(rowptr[-1])

    def odd(a, off):
        big = torch.zeros(len(a) + 8, dtype=torch.as_tensor(a).dtype, device=DEV)
        big[off:off + len(a)] = _dev(a)
        s = big[off:off + len(a)]
        assert s.data_ptr() % (2 * s.element_size()) == s.element_size()          # element-aligned and no more
        return s

    d_rowptr, d_col, d_val = odd(rowptr, 1), odd(col, 3), odd(val, 5)
    for v in (d_val, odd(val.astype(np.float32), 1)):
        got = _abi(d_rowptr, d_col, v, n_rows, 700, nnz)
        torch.cuda.synchronize()
        rp_t, col_t, val_t, order = TR.transpose(rowptr, col, val.astype(v.cpu().numpy().dtype), 700)
        assert np.array_equal(got[0].cpu().numpy(), rp_t) and np.array_equal(got[1].cpu().numpy(), col_t)
        assert np.array_equal(_bits(got[2].cpu().numpy()), _bits(val_t)) and np.array_equal(got[3].cpu().numpy(), order)
    # the inputs are not modified
    assert np.array_equal(d_rowptr.cpu().numpy(), rowptr) and np.array_equal(d_col.cpu().numpy(), col)
    assert np.array_equal(_bits(d_val.cpu().numpy()), _bits(val))


# ---- 6. round trip ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(300, 300, 9000), (40, 70000, 9000), (70000, 40, 9000)])
def test_twice_is_the_identity(shape):
    n_rows, n_cols, nnz = shape
    rowptr, col, val = TR.random_csr(np.random.default_rng(nnz + n_rows), n_rows, n_cols, nnz, unique=True)
    d = _dev(rowptr), _dev(col), _dev(val)
    rp_t, col_t, val_t, _ = _abi(*d, n_rows, n_cols, len(col))
    rp2, col2, val2, _ = _abi(rp_t, col_t, val_t, n_cols, n_rows, len(col))
    assert torch.equal(rp2, d[0]) and torch.equal(col2, d[1]) and torch.equal(val2.view(torch.int32), d[2].view(torch.int32))


# ---- 7. determinism and capture ---------------------------------------------------------------------------------------

def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(_BITS.get(x.dtype, x.dtype)), y.view(_BITS.get(y.dtype, y.dtype)))


def test_two_streams_give_the_same_bytes_and_the_call_is_capturable():
    """The call neither allocates nor synchronises: recorded in a graph (one linear chain) it replays to the bytes of the
    eager call, as test_gpu_layer_backward.py::test_one_call_is_capturable does for the backward."""
    rng = np.random.default_rng(21)
    rowptr, col, val = TR.random_csr(rng, 2000, 70000, 3 * _tile() + 77)           # three passes, four tiles
    d = _dev(rowptr), _dev(col), _dev(val)
    n_rows, n_cols, nnz = 2000, 70000, len(col)
    eager = _abi(*d, n_rows, n_cols, nnz)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _abi(*d, n_rows, n_cols, nnz)
    torch.cuda.synchronize()
    _same(eager, other)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = _abi(*d, n_rows, n_cols, nnz)
    for t in captured:
        t.fill_(-3)
    graph.replay()
    torch.cuda.synchronize()
    _same(eager, captured)
    rp_t, col_t, val_t, order = TR.transpose(rowptr, col, val, n_cols)
    assert np.array_equal(captured[3].cpu().numpy(), order) and np.array_equal(captured[0].cpu().numpy(), rp_t)


# ---- 8. ops.csr_transpose ---------------------------------------------------------------------------------------------

def _fixture_csrs():
    from _fixtures import load
    from sgracex1_amd import graphs
    for name in ("citeseer", "mol"):
        g = load(name)
        yield name + ".adj", graphs.csr_from_numpy(*g["adj"], g["N"], dtype=torch.float16)
        yield name + ".fea", graphs.csr_from_numpy(*g["fea"], g["M_fea"], dtype=torch.float32)
    yield "seeded", graphs.uniform_graph(3000, 40_000, seed=9, dtype=torch.float32, normalize=True)


def test_ops_device_method_equals_the_torch_method():
    from sgracex1_amd import ops
    seen_plan = set()
    for name, A in _fixture_csrs():
        A.validate()
        Td, od = ops.csr_transpose(A, return_order=True, method="device")
        Tt, ot = ops.csr_transpose(A, return_order=True, method="torch")
        assert (Td.n_rows, Td.n_cols, Td.nnz) == (Tt.n_rows, Tt.n_cols, Tt.nnz) == (A.n_cols, A.n_rows, A.nnz), name
        assert Td.val.dtype == Tt.val.dtype == A.val.dtype and od.dtype == ot.dtype == torch.int64
        assert torch.equal(Td.rowptr, Tt.rowptr) and torch.equal(Td.col, Tt.col) and torch.equal(od, ot), name
        assert torch.equal(Td.val.view(_BITS[Td.val.dtype]), Tt.val.view(_BITS[Tt.val.dtype])), name
        # the rule nnz >= 64 n_rows -> a plan, under either method
        assert (Td._plan is not None) == (Tt._plan is not None) == (Td.nnz >= 64 * Td.n_rows), name
        seen_plan.add(Td._plan is not None)
        plain = ops.csr_transpose(A, method="device")
        assert isinstance(plain, ops.Csr) and torch.equal(plain.col, Td.col)
        default = ops.csr_transpose(A)
        assert torch.equal(default.rowptr, Td.rowptr) and torch.equal(default.col, Td.col)
    assert seen_plan == {True, False}
    with pytest.raises(ValueError):
        ops.csr_transpose(A, method="host")


# ---- 9. the loader and the model --------------------------------------------------------------------------------------

def _example():
    spec = importlib.util.spec_from_file_location("sgrace_nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _planted(n=2000, seed=1):
    x, ei, y = _example().planted_partition(n, 5, 200, 0.02, 0.002, seed, DEV)
    train = torch.zeros(n, dtype=torch.bool, device=DEV)
    train[torch.randperm(n, generator=torch.Generator().manual_seed(1))[: n // 5].to(DEV)] = True
    return x, ei, y, train


def _loader(x, ei, y, train, **kw):
    from sgracex1_amd import pyg_lite
    return pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y, train_mask=train), [10, 10], batch_size=128, input_nodes=train,
                                   shuffle=True, seed=3, prepare="sym_norm2", **kw)


def _same_csr(a, b):
    assert (a.n_rows, a.n_cols, a.nnz) == (b.n_rows, b.n_cols, b.nnz)
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col[:a.nnz], b.col[:b.nnz])
    assert a.val.dtype == b.val.dtype and torch.equal(a.val[:a.nnz].view(_BITS[a.val.dtype]), b.val[:b.nnz].view(_BITS[b.val.dtype]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_transposed_batches_carry_the_three_attachments(dtype):
    from sgracex1_amd import ops
    x, ei, y, train = _planted()
    with pytest.raises(ValueError):
        from sgracex1_amd import pyg_lite
        pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y), [10], batch_size=8, transposed=True)       # needs prepare
    plain = iter(_loader(x, ei, y, train, dtype=dtype))
    for k, b in enumerate(_loader(x, ei, y, train, dtype=dtype, transposed=True)):
        p = next(plain)
        assert torch.equal(b.x, p.x) and torch.equal(b.n_id, p.n_id) and torch.equal(b.edge_index_agg, p.edge_index_agg)
        _same_csr(b.adj_norm, p.adj_norm)
        assert getattr(p.adj_norm, "_transpose_pattern", None) is None and ops.recorded(p.x, ("fea_csr_t", torch.float32)) is None
        fea = ops.recorded(b.x, ("fea_csr", torch.float32))
        fea_t = ops.recorded(b.x, ("fea_csr_t", torch.float32))
        assert fea is not None and fea_t is not None and fea.val.dtype == fea_t.val.dtype == torch.float32
        _same_csr(fea, ops.Csr.from_dense(b.x))
        if dtype == torch.float32:
            assert fea is ops.recorded(b.x, ("fea_csr", dtype))                   # the batch's own
        _same_csr(fea_t, ops.csr_transpose(fea, method="torch"))
        assert (fea_t._plan is not None) == (fea_t.nnz >= 64 * fea_t.n_rows)
        AT, order = b.adj_norm._transpose_pattern
        wantT, want_order = ops.csr_transpose(b.adj_norm, return_order=True, method="torch")
        _same_csr(AT, wantT)
        assert order.dtype == want_order.dtype and torch.equal(order, want_order)
        # feature_csr32 finds both and builds nothing
        Xc, Xt = ops.feature_csr32(b.x)
        assert Xc is fea and Xt is fea_t
        if k == 1:
            break


def _step_grads(batch, attention, accb, forbid_transpose, monkeypatch):
    from sgracex1_amd import config, ops, sgrace
    config.acc, config.device, config.compute_attention, config.accb = 1, "cuda", int(attention), int(accb)
    config.gat_edge_outputs = 1
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.float_type = 32, np.float32
    sgrace.init_SGRACE()
    torch.manual_seed(1)
    model = sgrace.GAT_PYNQ(batch.x.shape[1], 16, 1, 5).to(DEV).eval()            # eval: no dropout, the same net twice
    with monkeypatch.context() as m:
        if forbid_transpose:
            def refuse(*a, **k):
                raise AssertionError("ops.csr_transpose called during the step")
            m.setattr(ops, "csr_transpose", refuse)
        out = model(batch.x, batch.edge_index_agg)
        torch.nn.CrossEntropyLoss()(out[:batch.batch_size], batch.y[:batch.batch_size]).backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("attention,accb", [(0, 1), (1, 0)])
def test_a_step_on_a_transposed_batch_builds_no_transpose_and_gives_the_same_gradients(attention, accb, monkeypatch):
    """GCN under accb = 1 (grad_weights over the CSR of X^T) and GAT under accb = 0 (the transposed pattern): the step finds
    what the loader attached -- ops.csr_transpose raises if it is called -- and the gradients are the bits of the same batch
    from a loader without transposed=True, which builds the same arrays inside the step."""
    from sgracex1_amd import config, sgrace
    x, ei, y, train = _planted()
    old = config.snapshot()
    try:
        ready = next(iter(_loader(x, ei, y, train, transposed=True)))
        plain = next(iter(_loader(x, ei, y, train)))
        got = _step_grads(ready, attention, accb, True, monkeypatch)
        want = _step_grads(plain, attention, accb, False, monkeypatch)
        if attention:
            assert getattr(plain.adj_norm, "_transpose_pattern", None) is not None          # the step built it itself
        else:
            from sgracex1_amd import ops
            assert ops.recorded(plain.x, ("fea_csr_t", torch.float32)) is not None
        assert set(got) == set(want) and any("weight" in k for k in got)
        for k in want:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
            assert torch.isfinite(got[k]).all() and ((got[k] != 0).any() or "weight" not in k), k
    finally:
        config.restore(old)
        sgrace.init_SGRACE()


def test_example_with_device_batches_and_accb_learns(monkeypatch):
    """examples/sgrace_node_classification.py --device-batches --accb --batch-size 128 --num-neighbors 10,10, two epochs: the
    loader is asked for transposed batches and the mean training loss falls."""
    from sgracex1_amd import config, pyg_lite, sgrace
    mod = _example()
    asked = []
    real = pyg_lite.NeighborLoader

    class Spy(real):
        def __init__(self, *a, **kw):
            asked.append(kw.get("transposed"))
            super().__init__(*a, **kw)

    monkeypatch.setattr(pyg_lite, "NeighborLoader", Spy)
    old = config.snapshot()
    try:
        res, _, _ = mod.run(False, 32, epochs=2, acc=1, verbose=False, batch_size=128, num_neighbors=[10, 10],
                            device_batches=True, accb=1)
        print(res)
        assert asked == [True]
        first, second = res["epoch_loss"]
        assert np.isfinite(first) and second < first, res
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
