"""The entry-split GAT aggregate sgx_gat_aggregate_flat (csrc/gat_flat.hip) against float64 (_gat_ref.forward with its bound,
unchanged) on the graphs and masks of tests/_gat_flat_ref.py: every graph x mask x n_feat in {3, 8, 64, 100, 256} x fp16 /
fp32 x relu x the three dead-row rules.  D and the four statistics arrays are prefilled with NaN and fenced with sentinel
rows that must stay intact; every case runs twice and must give equal bits; the capacity cases give, on rows inside one
chunk, the bits of the same matrix at its exact entry count.  The statistics: score_row / score_col bit-equal to
sgx_gat_aggregate_stats's (no plan), row_max bit-equal to the maximum of the E_e that sgx_gat_edge_outputs forms from them,
row_sum within l rel_max; the S formed from them sums to 1 within (deg + 2) U on live rows and is dead_weight on dead ones.
Then: table pitches (unpadded, table_pitch, an odd pitch in fp16), the call recorded at capacity 3 T and replayed on another
matrix, and ops.gat_aggregate without keyword and fact bit for bit the direct sgx_gat_aggregate call it makes today."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _gat_flat_ref as R
import _gat_ref as G

pytestmark = pytest.mark.gpu
TDT = {"f16": torch.float16, "f32": torch.float32}
CODE = {"f16": 0, "f32": 1}
SENTINEL = -77.0
WIDTHS = [3, 8, 64, 100, 256]
RULES = ("zero", "mean", "fill")
DEAD_WEIGHT = {"zero": 0.0, "mean": 1.0 / R.N_COLS, "fill": 1.0 / R.N_NODES}


@functools.lru_cache(maxsize=None)
def T():
    from sgracex1_amd import _lib
    return _lib.lib.sgx_spmm_flat_chunk()


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@functools.lru_cache(maxsize=256)
def graph(name, mask, P, dt):
    return R.graph(name, mask, P, dt, T())


def to_dev(g, dt, capacity=None, pitch=None):
    """(rowptr, col, val, Wh, att, capacity); col / val hold `capacity` entries, those behind the real end poisoned: a column
    far outside the table and a NaN, never to be read.  Wh on rows `pitch` elements apart, the pad columns filled with 9."""
    cap = g["capacity"] if capacity is None else capacity
    nnz = len(g["col"])
    col = torch.full((max(cap, 1),), 1 << 30, dtype=torch.int32, device="cuda")
    val = torch.full((max(cap, 1),), float("nan"), dtype=TDT[dt], device="cuda")
    col[:nnz] = torch.as_tensor(g["col"], dtype=torch.int32)
    val[:nnz] = torch.as_tensor(g["val"]).to(TDT[dt])
    P = g["Wh"].shape[1]
    Wh = torch.full((g["n_cols"], P if pitch is None else pitch), 9.0, dtype=TDT[dt], device="cuda")
    Wh[:, :P] = torch.as_tensor(g["Wh"]).to(TDT[dt])
    att = torch.as_tensor(g["att"]).to(TDT[dt]).cuda()
    return torch.as_tensor(g["rowptr"], dtype=torch.int32, device="cuda"), col, val, Wh, att, cap


def run_flat(dt, dev, P, relu, rule, want_stats=True):
    """one call of the C entry point into NaN-filled outputs, each with a sentinel row behind the last; returns (D with its
    pad columns and sentinel row, the four statistics with their sentinel elements)"""
    from sgracex1_amd import _lib, ops
    rp, col, val, Wh, att, cap = dev
    n, N = rp.numel() - 1, Wh.shape[0]
    ldd = P + 5
    D = torch.full((n + 1, ldd), float("nan"), dtype=TDT[dt], device="cuda")
    D[n], D[:, P:] = SENTINEL, SENTINEL
    st = [torch.full((k + 1,), float("nan"), dtype=torch.float32, device="cuda") for k in (n, N, n, n)]
    for t in st:
        t[-1] = SENTINEL
    stats = _lib.GatStats(*(t.data_ptr() for t in st))
    fill = torch.as_tensor(R.fill_row(P)).cuda() if rule == "fill" else None
    n_nodes = {"zero": 0, "mean": N, "fill": R.N_NODES}[rule]
    sbytes = _lib.lib.sgx_gat_flat_scratch_bytes(cap, n, N, P, int(rule == "mean"))
    assert sbytes > 0
    scratch = torch.full((sbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    ops.check(_lib.lib.sgx_gat_aggregate_flat(CODE[dt], relu, n, N, P, 1, R.ALPHA, cap, rp.data_ptr(), col.data_ptr(), val.data_ptr(),
                                              Wh.data_ptr(), Wh.stride(0), att.data_ptr(), D.data_ptr(), ldd,
                                              fill.data_ptr() if fill is not None else None, n_nodes, scratch.data_ptr(), sbytes,
                                              ctypes.byref(stats) if want_stats else None,
                                              torch.cuda.current_stream().cuda_stream), "sgx_gat_aggregate_flat")
    return D, st


def aggregate_stats_scores(dt, dev, P):
    """score_row / score_col of sgx_gat_aggregate_stats without a plan on the same operands"""
    from sgracex1_amd import _lib, ops
    rp, col, val, Wh, att, _ = dev
    n, N = rp.numel() - 1, Wh.shape[0]
    D = torch.empty((n, P), dtype=TDT[dt], device="cuda")
    st = [torch.zeros((k,), dtype=torch.float32, device="cuda") for k in (n, N, n, n)]
    stats = _lib.GatStats(*(t.data_ptr() for t in st))
    s = torch.empty(_lib.lib.sgx_gat_scratch_bytes(N, P, 1, 0, None) // 4 + 64, dtype=torch.float32, device="cuda")
    ops.check(_lib.lib.sgx_gat_aggregate_stats(CODE[dt], 0, n, N, P, 1, R.ALPHA, rp.data_ptr(), col.data_ptr(), val.data_ptr(),
                                               Wh.data_ptr(), Wh.stride(0), att.data_ptr(), D.data_ptr(), P, None, 0, None,
                                               s.data_ptr(), ctypes.byref(stats), torch.cuda.current_stream().cuda_stream),
              "sgx_gat_aggregate_stats")
    return st[0], st[1]


def check_statistics(what, g, dt, dev, st, ref, rule):
    """the four arrays of one run against the float64 reference and against the calls that read them"""
    from sgracex1_amd import _lib, ops
    rp, col, val, Wh, att, cap = dev
    n, N = rp.numel() - 1, Wh.shape[0]
    nnz = len(g["col"])
    for t in st:
        assert float(t[-1]) == SENTINEL and not torch.isnan(t[:-1]).any(), what
    score_row, score_col, row_max, row_sum = (t[:-1] for t in st)
    want_row, want_col = aggregate_stats_scores(dt, dev, g["Wh"].shape[1])
    assert torch.equal(bits(score_row), bits(want_row)) and torch.equal(bits(score_col), bits(want_col)), what
    E = torch.full((max(cap, 1),), float("nan"), dtype=torch.float32, device="cuda")
    S = torch.full((max(cap, 1),), float("nan"), dtype=torch.float32, device="cuda")
    stats = _lib.GatStats(*(t.data_ptr() for t in st))
    ops.check(_lib.lib.sgx_gat_edge_outputs(CODE[dt], n, N, 1, R.ALPHA, rp.data_ptr(), col.data_ptr(), val.data_ptr(),
                                            ctypes.byref(stats), DEAD_WEIGHT[rule], E.data_ptr(), S.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "sgx_gat_edge_outputs")
    E, S = E[:nnz].cpu().numpy(), S[:nnz].double().cpu().numpy()
    live, dead, rowptr = ref["live"], ref["dead"], g["rowptr"]
    m = G._seg(np.maximum, np.where(live, E, np.float32(-np.inf)).astype(np.float32), rowptr, np.float32(-np.inf))
    m[dead] = 0.0
    assert np.array_equal(row_max.cpu().numpy().view(np.int32), m.astype(np.float32).view(np.int32)), what
    l, rel_max = R.rel_of(g, ref)
    got_l = row_sum.double().cpu().numpy()
    assert (got_l[dead] == 0).all() and (np.abs(got_l - l) <= l * rel_max)[~dead].all(), what
    sums = G._seg(np.add, S, rowptr, 0.0)
    deg = np.diff(rowptr)
    assert (np.abs(sums - 1.0) <= (deg + 2) * G.U)[~dead].all(), (what, np.abs(sums - 1.0)[~dead].max())
    if dead.any() and nnz:
        assert (S[dead[ref["row"]]] == np.float32(DEAD_WEIGHT[rule])).all(), what


def check_case(name, mask, dt, P, pitch=None, stats_on=("zero",)):
    g = graph(name, mask, P, dt)
    dev = to_dev(g, dt, pitch=pitch)
    exact = to_dev(g, dt, capacity=len(g["col"]), pitch=pitch) if g["capacity"] > len(g["col"]) else None
    n = g["n_rows"]
    rp = g["rowptr"]
    inside = torch.as_tensor(rp[:-1] // T() == (np.maximum(rp[1:], 1) - 1) // T(), device="cuda")
    for rule in RULES:
        for relu in (0, 1):
            what = f"{name} {mask} {dt} P={P} pitch={pitch} relu={relu} {rule}"
            D, st = run_flat(dt, dev, P, relu, rule)
            again, st2 = run_flat(dt, dev, P, relu, rule)
            assert torch.equal(bits(D), bits(again)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(st, st2)), \
                f"{what}: two runs differ"
            got = D.double().cpu().numpy()
            assert (got[:n, P:] == SENTINEL).all() and (got[n] == SENTINEL).all(), f"{what}: a store outside the rows of D"
            ref = R.reference(g, dt, relu, rule)
            G.check(what, got[:n, :P], ref["D"], ref["bD"], np.arange(n), {})
            if exact is not None:
                De, _ = run_flat(dt, exact, P, relu, rule)
                assert torch.equal(bits(D[:n, :P][inside]), bits(De[:n, :P][inside])), f"{what}: capacity changes the bits"
            if rule in stats_on and relu == 0:
                check_statistics(what, g, dt, dev, st, ref, rule)
                Dn, _ = run_flat(dt, dev, P, relu, rule, want_stats=False)         # without statistics: the same D
                assert torch.equal(bits(D), bits(Dn)), what


@pytest.mark.parametrize("P", WIDTHS)
@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_rule_on_every_graph_and_mask(dt, P):
    for name in R.degree_cases(T()):
        for mask in R.MASKS:
            check_case(name, mask, dt, P, stats_on=RULES if name in ("masked_chunks", "long_middle") else ("zero",))


@pytest.mark.parametrize("dt,P,pitch", [("f16", 100, 100), ("f16", 100, None), ("f16", 3, 3), ("f16", 41, 43), ("f32", 100, None),
                                         ("f32", 3, 3), ("f32", 41, 41)])
def test_table_pitches(dt, P, pitch):
    """unpadded rows (a dword pitch, or odd halves in fp16: one element per lane), and the library's own table_pitch"""
    from sgracex1_amd import ops
    pitch = ops.table_pitch(P, 2 if dt == "f16" else 4) if pitch is None else pitch
    for name in ("nnz_T+1", "long_middle", "ends_on_chunk_end", "empty_run", "capacity", "masked_chunks"):
        for mask in ("third", "chunks", "descend"):
            check_case(name, mask, dt, P, pitch=pitch)


# ---- ops.gat_aggregate: the keyword, the fact, the replay, the default -------------------------------------------------------

def _csr(g, dt, capacity=None):
    from sgracex1_amd import ops
    rp, col, val, _, _, _ = to_dev(g, dt, capacity=capacity)
    nnz = len(g["col"])
    col[nnz:], val[nnz:] = 0, 0
    return ops.Csr(rp, col, val, g["n_cols"])


def test_keyword_and_fact_take_the_flat_form():
    from sgracex1_amd import ops
    g = graph("masked_chunks", "third", 64, "f16")
    dev = to_dev(g, "f16")
    Wh, att = dev[3], dev[4]
    direct, st = run_flat("f16", dev, 64, 1, "mean")
    A = _csr(g, "f16")
    out, stats = ops.gat_aggregate(A, Wh, att, alpha=R.ALPHA, relu=True, fill_dead_rows=True, want_row_stats=True, schedule="flat")
    assert torch.equal(bits(out), bits(direct[:-1, :64]))
    assert all(torch.equal(bits(a), bits(b[:-1])) for a, b in zip(stats.tensors(), st))
    B = _csr(g, "f16").with_facts(flat=True)
    assert torch.equal(bits(ops.gat_aggregate(B, Wh, att, alpha=R.ALPHA, relu=True, fill_dead_rows=True)), bits(out))
    assert B._plan is None
    fill = torch.as_tensor(R.fill_row(64)).cuda()
    by_fill = ops.gat_aggregate(B, Wh, att, alpha=R.ALPHA, relu=True, fill_row=fill, n_nodes=R.N_NODES)
    assert torch.equal(bits(by_fill), bits(run_flat("f16", dev, 64, 1, "fill")[0][:-1, :64]))
    # a flat-marked matrix with arguments the form does not support runs as it does without the fact
    want = ops.gat_aggregate(_csr(g, "f16"), Wh, att, alpha=R.ALPHA, fill_dead_rows=False, want_edge_outputs=True)
    got = ops.gat_aggregate(B, Wh, att, alpha=R.ALPHA, fill_dead_rows=False, want_edge_outputs=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))
    att2 = torch.cat([att[:32], att[64:96], att[32:64], att[96:]])
    assert torch.equal(bits(ops.gat_aggregate(B, Wh, att2, alpha=R.ALPHA, fill_dead_rows=False, heads=2)),
                       bits(ops.gat_aggregate(_csr(g, "f16"), Wh, att2, alpha=R.ALPHA, fill_dead_rows=False, heads=2)))


def test_recorded_call_replays_on_another_matrix():
    """recorded at capacity 3 T on a side stream after a warm-up, under sync-debug "error"; then rowptr, col and val are
    overwritten in place with a matrix of another row pointer and other values: the replay equals an eager call on it"""
    from sgracex1_amd import ops
    first, second = graph("capacity", "third", 64, "f16"), graph("capacity_exact_end", "chunks", 64, "f16")
    cap = 3 * T()
    n = max(first["n_rows"], second["n_rows"])

    def padded(g):                                       # the same row count for both: empty rows behind the last
        rp = np.concatenate([g["rowptr"], np.full(n - g["n_rows"], g["rowptr"][-1])])
        return dict(g, rowptr=rp, n_rows=n)

    first, second = padded(first), padded(second)
    assert len(first["col"]) <= cap and len(second["col"]) <= cap and len(first["col"]) != len(second["col"])
    A = _csr(first, "f16", capacity=cap)
    _, _, _, Wh, att, _ = to_dev(first, "f16")
    Wh2, att2 = to_dev(second, "f16")[3:5]
    out = torch.empty((n, 64), dtype=torch.float16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gat_aggregate(A, Wh, att, alpha=R.ALPHA, relu=True, fill_dead_rows=True, out=out, schedule="flat")   # warm-up: sizes the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_first = out.clone()
    graph_ = torch.cuda.CUDAGraph()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.graph(graph_, stream=side):
            ops.gat_aggregate(A, Wh, att, alpha=R.ALPHA, relu=True, fill_dead_rows=True, out=out, schedule="flat")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert A._plan is None
    out.fill_(SENTINEL)
    graph_.replay()
    assert torch.equal(bits(out), bits(eager_first))
    nnz2 = len(second["col"])
    A.rowptr.copy_(torch.as_tensor(second["rowptr"], dtype=torch.int32))
    A.col[:nnz2] = torch.as_tensor(second["col"], dtype=torch.int32).cuda()
    A.col[nnz2:] = 1 << 30                                               # what lies behind the new end is never read
    A.val[:nnz2] = torch.as_tensor(second["val"]).half().cuda()
    A.val[nnz2:] = float("nan")
    Wh.copy_(Wh2)
    att.copy_(att2)
    out.fill_(SENTINEL)
    graph_.replay()
    replayed = out.clone()
    eager = ops.gat_aggregate(_csr(second, "f16", capacity=cap), Wh, att, alpha=R.ALPHA, relu=True, fill_dead_rows=True,
                              schedule="flat")
    assert torch.equal(bits(replayed), bits(eager))
    ref = R.reference(second, "f16", 1, "mean")
    G.check("replay on the second matrix", replayed.double().cpu().numpy(), ref["D"], ref["bD"], np.arange(n), {})


@pytest.mark.parametrize("rule", ["zero", "mean", "fill"])
def test_default_call_is_unchanged(rule):
    """without keyword and fact: the bits of the direct sgx_gat_aggregate / sgx_gat_aggregate_fill call made today (a small
    matrix: no plan), and the flat form beside it inside the bound"""
    from sgracex1_amd import _lib, ops
    g = graph("mixed", "third", 64, "f16")
    dev = to_dev(g, "f16")
    rp, col, val, Wh, att, _ = dev
    A = _csr(g, "f16")
    assert not A._flat and not A.wants_plan
    n, N = g["n_rows"], g["n_cols"]
    fill = torch.as_tensor(R.fill_row(64)).cuda() if rule == "fill" else None
    kw = dict(fill_row=fill, n_nodes=R.N_NODES) if rule == "fill" else dict(fill_dead_rows=rule == "mean")
    got = ops.gat_aggregate(A, Wh, att, alpha=R.ALPHA, relu=True, **kw)
    assert A._plan is None
    D = torch.full((n, 64), SENTINEL, dtype=torch.float16, device="cuda")
    s = torch.empty(_lib.lib.sgx_gat_scratch_bytes(N, 64, 1, int(rule == "mean"), None) // 4 + 64, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if rule == "fill":
        ops.check(_lib.lib.sgx_gat_aggregate_fill(0, 1, n, N, 64, 1, R.ALPHA, rp.data_ptr(), A.col.data_ptr(), A.val.data_ptr(),
                                                  Wh.data_ptr(), 64, att.data_ptr(), D.data_ptr(), 64, None, None, fill.data_ptr(),
                                                  R.N_NODES, None, s.data_ptr(), stream), "sgx_gat_aggregate_fill")
    else:
        ops.check(_lib.lib.sgx_gat_aggregate(0, 1, int(rule == "mean"), n, N, 64, 1, R.ALPHA, rp.data_ptr(), A.col.data_ptr(),
                                             A.val.data_ptr(), Wh.data_ptr(), 64, att.data_ptr(), D.data_ptr(), 64, None, None, None,
                                             s.data_ptr(), stream), "sgx_gat_aggregate")
    assert torch.equal(bits(got), bits(D))
    flat = ops.gat_aggregate(A, Wh, att, alpha=R.ALPHA, relu=True, schedule="flat", **kw)
    ref = R.reference(g, "f16", 1, rule)
    G.check("flat beside the default", flat.double().cpu().numpy(), ref["D"], ref["bD"], np.arange(n), {})
