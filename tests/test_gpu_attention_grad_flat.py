"""The attention gradient by stored entries, sgx_gat_attention_grad_flat (csrc/gat_attention_grad_flat.hip), against
float64 on the smallest graphs at which its rule can fail (tests/_attention_grad_flat_ref.py: T = sgx_spmm_flat_chunk();
end in {0, 1, T - 1, T, T + 1, 3T + 5}, a hub row over 3T, runs of empty rows first, in the middle and last, fewer than T
rows and 2T + 3 rows), at F in {3, 8, 64, 100, 256}, with Wh on 16 bytes (the vector arm) and on an odd pitch one float off
(the element-wise arm).

Bound, derived and not measured: each output element is an fp32 sum whose longest addition chain is d = T L / 64 (inside a
lane group) + 64 / L (the groups) + ceil(chunks / 16) + 16 (the second launch), so it lies within (d + 2) 2^-24 sum |term|
of float64 (_attention_grad_flat_ref.bound computes d from T, L and the chunk count of the half).  sgx_gat_attention_grad
sums the same terms in another order whose chains are no longer: the two agree within twice the bound.
Every case: equal bits on two runs; equal bits at capacity = end, end + 1 and end + 3T with NaN weights and columns far
outside the table behind the end; sentinels around grad_attention and the workspace (itself prefilled with NaN).  Then the
call recorded at capacity 3T and replayed on a second matrix inside it, under sync-debug "error"."""
import functools

import numpy as np
import pytest
import torch

import _attention_grad_flat_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = [3, 8, 12, 20, 64, 100, 256]
SENTINEL = -77.0
GUARD = 64                    # sentinel floats on either side of an output and of the workspace


@functools.lru_cache(maxsize=None)
def T():
    from sgracex1_amd import _lib
    return _lib.lib.sgx_spmm_flat_chunk()


@functools.lru_cache(maxsize=None)
def graph(name):
    deg = R.degree_cases(T())[name]
    n_cols = max(len(deg), 50) + 3
    return R.build(deg, n_cols, seed=len(name)), n_cols


@functools.lru_cache(maxsize=None)
def table(n_cols, F):
    return (np.random.default_rng(1000 + F).random((n_cols, F)) * 2 - 1).astype(np.float32)


def table_dev(Wh, aligned):
    """aligned: rows of ceil(F / 4) * 4 floats on 16 bytes; else rows of an odd pitch that start one float off"""
    n, F = Wh.shape
    pitch = -(-F // 4) * 4 if aligned else (F + 1) | 1
    buf = torch.full((n * pitch + 5,), 9.0, dtype=torch.float32, device="cuda")
    off = 0 if aligned else 1
    view = buf[off:off + n * pitch].view(n, pitch)
    view[:, :F] = torch.as_tensor(Wh)
    assert (view.data_ptr() % 16 == 0) == aligned
    return view


def device_graph(g, capacity):
    rp, ci, sg, g1 = g
    col = torch.full((max(capacity, 1),), 1 << 30, dtype=torch.int32, device="cuda")
    w = torch.full((max(capacity, 1),), float("nan"), dtype=torch.float32, device="cuda")
    col[:len(ci)] = torch.as_tensor(ci)
    w[:len(ci)] = torch.as_tensor(sg)
    return torch.as_tensor(rp, dtype=torch.int32, device="cuda"), col, w, torch.as_tensor(g1, device="cuda")


def run_flat(dg, capacity, n_cols, Wd, F):
    """one call of the C entry point between sentinels; returns grad_attention [2 F]"""
    from sgracex1_amd import _lib, ops
    rp, col, w, g1 = dg
    n = rp.numel() - 1
    out = torch.full((2 * F + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    need = _lib.lib.sgx_gat_attention_grad_flat_workspace_bytes(capacity, n, F)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need // 4 + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert ws.data_ptr() % 256 == 0 and (GUARD * 4) % 256 == 0
    ws[GUARD:GUARD + need // 4] = float("nan")
    ops.check(_lib.lib.sgx_gat_attention_grad_flat(n, n_cols, F, capacity, rp.data_ptr(), col.data_ptr(), w.data_ptr(), g1.data_ptr(),
                                                   Wd.data_ptr(), Wd.stride(0), out[GUARD:].data_ptr(), ws[GUARD:].data_ptr(), need,
                                                   torch.cuda.current_stream().cuda_stream), "sgx_gat_attention_grad_flat")
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + 2 * F:] == SENTINEL).all(), "a store outside grad_attention"
    assert (ws[:GUARD] == SENTINEL).all() and (ws[GUARD + need // 4:] == SENTINEL).all(), "a store outside the workspace"
    return out[GUARD:GUARD + 2 * F].clone()


def bits(t):
    return t.contiguous().view(torch.int32)


def check_case(name, F, aligned):
    from sgracex1_amd import ops
    g, n_cols = graph(name)
    rp, ci, sg, g1 = g
    end, t = int(rp[-1]), T()
    Wh = table(n_cols, F)
    Wd = table_dev(Wh, aligned)
    got = run_flat(device_graph(g, end), end, n_cols, Wd, F)
    assert torch.equal(bits(got), bits(run_flat(device_graph(g, end), end, n_cols, Wd, F))), f"{name} F={F}: two runs differ"
    for cap in (end + 1, end + 3 * t):
        assert torch.equal(bits(got), bits(run_flat(device_graph(g, cap), cap, n_cols, Wd, F))), f"{name} F={F}: capacity {cap} shows"
    want, mag = R.exact(rp, ci, sg, g1, Wh)
    bound = R.bound(rp, t, F, mag)
    err = np.abs(got.double().cpu().numpy() - want)
    assert (err <= bound).all(), f"{name} F={F} aligned={aligned}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}"
    if end == 0:
        assert not bits(got[F:]).any(), f"{name}: the entries' half of a matrix without entries is +0"
    # the row-owning call on the same inputs: the same terms in another order
    A = ops.Csr(torch.as_tensor(rp, dtype=torch.int32, device="cuda"), torch.as_tensor(ci, device="cuda"),
                torch.zeros(end, dtype=torch.float32, device="cuda"), n_cols)
    rows = ops.gat_attention_grad(A, torch.as_tensor(sg, device="cuda") if end else torch.zeros(1, device="cuda"),
                                  torch.as_tensor(g1, device="cuda"), Wd[:, :F])
    assert (np.abs(rows.double().cpu().numpy() - got.double().cpu().numpy()) <= 2 * bound).all(), f"{name} F={F}: the two calls disagree"


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "elementwise"])
def test_rule_on_every_graph(F, aligned):
    for name in R.degree_cases(T()):
        check_case(name, F, aligned)


def test_no_rows_and_zero_weights_give_plus_zero():
    from sgracex1_amd import _lib, ops
    F = 8
    out = torch.full((2 * F,), SENTINEL, dtype=torch.float32, device="cuda")
    need = _lib.lib.sgx_gat_attention_grad_flat_workspace_bytes(0, 0, F)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    ops.check(_lib.lib.sgx_gat_attention_grad_flat(0, 0, F, 0, None, None, None, None, None, F, out.data_ptr(), ws.data_ptr(), need,
                                                   torch.cuda.current_stream().cuda_stream), "n_rows = 0")
    assert not bits(out).any()
    g, n_cols = graph("end_0")
    rp, ci, sg, g1 = g
    got = run_flat(device_graph((rp, ci, sg, np.zeros_like(g1)), 5), 5, n_cols, table_dev(table(n_cols, F), True), F)
    assert not bits(got).any()


def test_keyword_and_fact_take_the_flat_call():
    from sgracex1_amd import ops
    g, n_cols = graph("hub")
    rp, ci, sg, g1 = g
    F = 64
    Wd = table_dev(table(n_cols, F), True)
    direct = run_flat(device_graph(g, len(ci)), len(ci), n_cols, Wd, F)
    mk = lambda: ops.Csr(torch.as_tensor(rp, dtype=torch.int32, device="cuda"), torch.as_tensor(ci, device="cuda"),
                         torch.zeros(len(ci), dtype=torch.float32, device="cuda"), n_cols)
    s, r = torch.as_tensor(sg, device="cuda"), torch.as_tensor(g1, device="cuda")
    assert torch.equal(bits(ops.gat_attention_grad(mk(), s, r, Wd, schedule="flat")), bits(direct))
    marked = mk().with_facts(flat=True)
    assert torch.equal(bits(ops.gat_attention_grad(marked, s, r, Wd)), bits(direct)) and marked._plan is None
    with pytest.raises(ValueError):
        ops.gat_attention_grad(mk(), s, r, Wd, schedule="rows")


def test_recorded_call_replays_on_a_second_matrix_inside_the_capacity():
    from sgracex1_amd import ops
    t, F = T(), 64
    cap = 3 * t
    first = [5, 2 * t + 9] + [3] * 40 + [0] * 10                              # a hub row that crosses two chunk ends
    second = [1] * 30 + [0] * 5 + [t + 17] + [2] * 16                         # another profile, fewer entries
    assert len(first) == len(second) and sum(first) <= cap and sum(second) < sum(first) - t // 2
    n_cols = len(first) + 9
    g1_, g2_ = R.build(first, n_cols, seed=1), R.build(second, n_cols, seed=2)
    Wd = table_dev(table(n_cols, F), True)
    rp, col, w, r = device_graph(g1_, cap)
    A = ops.Csr(rp, col, torch.zeros(cap, dtype=torch.float32, device="cuda"), n_cols).with_facts(flat=True)
    assert A.nnz == cap
    eager_first = ops.gat_attention_grad(A, w, r, Wd)                           # sizes the workspace outside the recording
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.graph(graph_):
            out = ops.gat_attention_grad(A, w, r, Wd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    graph_.replay()
    assert torch.equal(bits(out), bits(eager_first))
    rp2, ci2, sg2, r2 = g2_
    rp.copy_(torch.as_tensor(rp2, dtype=torch.int32))
    col[:len(ci2)] = torch.as_tensor(ci2).cuda()
    col[len(ci2):] = 1 << 30
    w[:len(ci2)] = torch.as_tensor(sg2).cuda()
    w[len(ci2):] = float("nan")
    r.copy_(torch.as_tensor(r2))
    graph_.replay()
    replayed = out.clone()
    exact_cap = run_flat(device_graph(g2_, len(ci2)), len(ci2), n_cols, Wd, F)
    assert torch.equal(bits(replayed), bits(exact_cap))
    want, mag = R.exact(rp2, ci2, sg2, r2, table(n_cols, F))
    assert (np.abs(replayed.double().cpu().numpy() - want) <= R.bound(rp2, t, F, mag)).all()
