"""The kernels of the attention layer's backward on every lane-group arm, each against float64 on the graphs of
tests/_gat_bwd_graphs.py (tests/test_gat_bwd_arms_cpu.py holds the record of which width reaches which arm):

  edge pass, E / S form        sgx_gat_backward_edges at every width of EDGE_WIDTHS, both value types, G on 16 bytes and
                               4 bytes off them on an odd pitch (g_vec = 0), dead rows with and without dead / dead_row_sum.
                               E and S are the float64 forward's, rounded to fp32; every element inside the bounds of
                               _gat_ref.backward_edges.  Pad columns of Wh and G hold NaN; the index and value arrays run
                               on behind rowptr[n_rows] with columns outside the table and NaN; sg and g1 lie between
                               sentinels, which come back untouched like sg's own tail; the same bits on a second run.
  edge pass, statistics form   sgx_gat_backward_edges_stats on the same widths through test_gpu_gat_stats'
                               check_backward_from_statistics, on statistics formed from the float64 forward.  The graph
                               is the one without the deliberate zero scores: fp32 statistics cannot carry them.
  attention gradient           sgx_gat_attention_grad (rows) and sgx_gat_attention_grad_flat (stored entries) at every
                               width of ATTENTION_WIDTHS on a padded pitch (16-byte gathers) and an odd pitch one float off
                               (element gathers), NaN in the pad columns, sg and g1 arbitrary.

Bounds, derived and not measured.  The edge pass: _gat_ref.backward_edges' own, plus check_backward_from_statistics' terms
for the weights formed again.  The entry-split form: _attention_grad_flat_ref.bound.  The row form: (d + 2) 2^-24 times the
sum of the magnitudes of an element's terms (|Wh|^T |g1|, |Wh|^T colsum |sg|), d the longest addition chain of the kernel's
order (_gat_bwd_graphs.attention_depth): an fma chain of at most 256 per row or chunk, the chunks of a long row in chunk
order or the rows of a worker's share and the WORKERS partials, an addition per long row of the run, the slices.  The
factor is at least 3 x 2^-24 = 1.8e-7, so it is never below test_gpu_layer_grad's TOL["grad_attention"] = 1e-7 (which
multiplies a far looser magnitude): the derived bound is the one used throughout.  Every case prints its worst error / bound."""
import functools

import numpy as np
import pytest
import torch

import _attention_grad_flat_ref as FR
import _gat_bwd_graphs as B
import _gat_ref as R

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")
DT = {"f16": torch.float16, "f32": torch.float32}
SENTINEL = -77.0
GUARD = 64
RULES = ("zero", "mean")                 # dead rows: S = 0 and no dead / dead_row_sum; S = 1 / n_cols and both given


@functools.lru_cache(maxsize=None)
def graph(kind, dt="f32", zero_scores=True):
    if kind == "adversarial":
        return B.adversarial(dt, zero_scores=zero_scores)
    if kind == "many_entries":
        return B.many_entries(torch.cuda.get_device_properties(0).multi_processor_count)
    if kind == "many_rows":
        return B.many_rows()
    if kind == "hub_wide":
        return B.hub(B.MANY_ROWS)
    if kind == "hub":
        return B.hub(300)
    return {"tiny": B.tiny, "no_entries": B.no_entries}[kind](dt)


@functools.lru_cache(maxsize=None)
def forward(kind, dt, zero_scores, rule):
    """the float64 forward on the graph's scores, and its E and S as the fp32 arrays the backward is handed"""
    ref = B.forward_ref(graph(kind, dt, zero_scores), rule)
    return ref, ref["E"].astype(np.float32), ref["S"].astype(np.float32)


@functools.lru_cache(maxsize=8)
def edge_reference(kind, dt, F, rule):
    g = graph(kind, dt)
    ref, E32, S32 = forward(kind, dt, True, rule)
    Wh, G = B.edge_tables(g, F)
    dead = ref["dead"] if rule == "mean" else None
    return Wh, G, dead, R.backward_edges(g, E32, S32, G, Wh, dead=dead)


def padded(a, aligned, pad=4):
    """a [n, F] fp32 on the device in rows with NaN pad columns: a pitch of ceil(F / 4) * 4 + pad floats on 16 bytes, or
    an odd pitch starting one float off 16 bytes.  Returns the [n, F] view."""
    n, F = a.shape
    pitch = -(-F // 4) * 4 + pad if aligned else (F + 1) | 1
    off = 0 if aligned else 1
    buf = torch.full((n * pitch + 8,), float("nan"), dtype=torch.float32, device=dev)
    view = buf[off:off + n * pitch].view(n, pitch)
    view[:, :F] = torch.as_tensor(a, dtype=torch.float32)
    assert (view.data_ptr() % 16 == 0 and pitch % 4 == 0) == aligned and pitch > F
    return view[:, :F]


@functools.lru_cache(maxsize=None)
def device_graph(kind, dt):
    """rowptr, and col / val at the capacity: columns outside the table and NaN values behind rowptr[n_rows]"""
    g = graph(kind, dt)
    return (torch.as_tensor(g["rowptr"], dtype=torch.int32, device=dev), torch.as_tensor(g["col_cap"], dtype=torch.int32, device=dev),
            torch.as_tensor(g["val_cap"]).to(DT[dt]).to(dev))


def at_capacity(a, capacity):
    out = torch.full((capacity,), float("nan"), dtype=torch.float32, device=dev)
    out[:len(a)] = torch.as_tensor(a, dtype=torch.float32)
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def run_edges(kind, dt, F, E32, S32, Gd, Whd, dead, dead_rs):
    """one call of sgx_gat_backward_edges with sg and g1 between sentinels; returns (sg [nnz], g1 [n_rows])"""
    from sgracex1_amd import _lib, ops
    g = graph(kind, dt)
    rowptr, col, val = device_graph(kind, dt)
    n, nnz, cap = g["n_rows"], g["nnz"], g["capacity"]
    sg = torch.full((cap + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    g1 = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    E, S = at_capacity(E32, cap), at_capacity(S32, cap)
    dead_t = None if dead is None else torch.as_tensor(dead, device=dev).to(torch.uint8)
    ptr = lambda t: None if t is None else t.data_ptr()
    ops.check(_lib.lib.sgx_gat_backward_edges(ops.dtype_code(DT[dt]), n, g["n_cols"], F, 0.2, rowptr.data_ptr(), col.data_ptr(),
                                              val.data_ptr(), E.data_ptr(), S.data_ptr(), Gd.data_ptr(), Gd.stride(0), Whd.data_ptr(),
                                              Whd.stride(0), ptr(dead_t), ptr(dead_rs), sg[GUARD:].data_ptr(), g1[GUARD:].data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "sgx_gat_backward_edges")
    assert (sg[:GUARD] == SENTINEL).all() and (sg[GUARD + nnz:] == SENTINEL).all(), "a store outside sg[0 : nnz]"
    assert (g1[:GUARD] == SENTINEL).all() and (g1[GUARD + n:] == SENTINEL).all(), "a store outside g1"
    return sg[GUARD:GUARD + nnz].clone(), g1[GUARD:GUARD + n].clone()


def ratio(got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - want)
    return float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0


def check_edges(kind, dt, F, aligned):
    g = graph(kind, dt)
    row = R.rows_of(g["rowptr"])
    for rule in RULES:
        Wh, G, dead, (want_sg, want_g1, b_sg, b_g1) = edge_reference(kind, dt, F, rule)
        _ref, E32, S32 = forward(kind, dt, True, rule)
        Whd, Gd = padded(Wh, True), padded(G, aligned)
        dead_rs = None if dead is None else torch.as_tensor((G @ Wh.mean(0)).astype(np.float32), device=dev)
        sg, g1 = run_edges(kind, dt, F, E32, S32, Gd, Whd, dead, dead_rs)
        sg2, g12 = run_edges(kind, dt, F, E32, S32, Gd, Whd, dead, dead_rs)
        assert torch.equal(bits(sg), bits(sg2)) and torch.equal(bits(g1), bits(g12)), "not the same bits on a second run"
        sg, g1 = sg.double().cpu().numpy(), g1.double().cpu().numpy()
        print("edges", kind, dt, F, "g_vec" if aligned else "g_elem", rule, f"sg {ratio(sg, want_sg, b_sg):.3g}",
              f"g1 {ratio(g1, want_g1, b_g1):.3g} of the bound")
        R.check(f"sg {kind} {rule}", sg, want_sg, b_sg, row, g["names"])
        R.check(f"g1 {kind} {rule}", g1, want_g1, b_g1, np.arange(g["n_rows"]), g["names"])


@pytest.mark.parametrize("aligned", [True, False], ids=["g_vec", "g_elem"])
@pytest.mark.parametrize("F", B.EDGE_WIDTHS)
@pytest.mark.parametrize("dt", list(DT))
def test_edge_pass_from_E_and_S(dt, F, aligned):
    check_edges("adversarial", dt, F, aligned)
    check_edges("tiny", dt, F, aligned)


@pytest.mark.parametrize("dt", list(DT))
def test_edge_pass_without_entries(dt):
    """n_rows > 0 and not one stored entry: g1 is +0 bit for bit and sg is not written"""
    g = graph("no_entries", dt)
    F = 17
    Wh, G = B.edge_tables(g, F)
    none = np.zeros(0, np.float32)
    for aligned in (True, False):
        sg, g1 = run_edges("no_entries", dt, F, none, none, padded(G, aligned), padded(Wh, True), None, None)
        assert sg.numel() == 0 and not bits(g1).any()


def test_edge_pass_past_one_sweep_of_the_persistent_grid():
    g = graph("many_entries")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert g["nnz"] > B.DOT_BLOCK * B.DOT_BLOCKS_PER_CU * cus
    check_edges("many_entries", "f32", 20, True)


@pytest.mark.parametrize("F", B.EDGE_WIDTHS)
@pytest.mark.parametrize("dt", list(DT))
def test_edge_pass_from_statistics(dt, F):
    """sg, g1 and S_out of sgx_gat_backward_edges_stats; G is contiguous there, so its alignment arm follows F."""
    from sgracex1_amd import ops
    from test_gpu_gat_stats import check_backward_from_statistics
    for kind in ("adversarial", "tiny"):
        g = graph(kind, dt, False)
        Wh, _G = B.edge_tables(g, F)
        Whd = padded(Wh, True)
        f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)
        i32 = lambda a: torch.as_tensor(a, dtype=torch.int32, device=dev)
        A = ops.Csr(i32(g["rowptr"]), i32(g["col"]), torch.as_tensor(g["val"]).to(DT[dt]).to(dev), g["n_cols"])
        for rule in RULES:
            ref, _E, _S = forward(kind, dt, False, rule)
            m, l = B.row_statistics(g, ref)
            stats = ops.GatStats.of(f32(g["score_row"]), f32(g["score_col"]), f32(m), f32(l))
            check_backward_from_statistics(dict(g, Wh=Wh), ref, A, stats, Whd, F, rule == "mean",
                                           1.0 / g["n_cols"] if rule == "mean" else 0.0, (kind, dt, F, rule))


# ---- the attention gradient ------------------------------------------------------------------------------------------------

AG_GRAPHS = {"adversarial": lambda F: True, "many_rows": lambda F: F <= 20, "hub_wide": lambda F: F == 4, "hub": lambda F: F == 64}


@functools.lru_cache(maxsize=None)
def ag_inputs(kind):
    """(graph, sg at the capacity with NaN behind nnz, g1) and the same on the device"""
    g = graph(kind)
    sg, g1 = B.attention_inputs(g["rowptr"], g["col_cap"], g["nnz"], seed=len(kind))
    rowptr, col, _val = device_graph(kind, "f32")
    return g, sg, g1, (rowptr, col, torch.as_tensor(sg, device=dev), torch.as_tensor(g1, device=dev))


@functools.lru_cache(maxsize=4)
def ag_reference(kind, F):
    g, sg, g1, _d = ag_inputs(kind)
    Wh = np.random.default_rng([F, 23]).uniform(-1, 1, (g["n_cols"], F)).astype(np.float32)
    want, mag = FR.exact(g["rowptr"], g["col"], sg, g1, Wh)
    return Wh, want, mag


def ag_cases(F):
    return [k for k, takes in AG_GRAPHS.items() if takes(F)]


@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "elementwise"])
@pytest.mark.parametrize("F", B.ATTENTION_WIDTHS)
def test_attention_grad_by_rows(F, aligned):
    from sgracex1_amd import ops
    for kind in ag_cases(F):
        g, _sg, _g1, (rowptr, col, sg_d, g1_d) = ag_inputs(kind)
        Wh, want, mag = ag_reference(kind, F)
        Whd = padded(Wh, aligned)
        A = ops.Csr(rowptr, col, torch.zeros(g["capacity"], dtype=torch.float32, device=dev), g["n_cols"])
        got = ops.gat_attention_grad(A, sg_d, g1_d, Whd)
        assert torch.equal(bits(got), bits(ops.gat_attention_grad(A, sg_d, g1_d, Whd))), "not the same bits on a second run"
        bound = B.attention_bound(F, g["rowptr"], mag)
        r = ratio(got.double().cpu().numpy(), want, bound)
        print("attention_grad rows", kind, F, "vec" if aligned else "elementwise", "depth", B.attention_depth(F, g["rowptr"]),
              f"worst error / bound {r:.3g}")
        assert torch.isfinite(got).all() and r <= 1.0, (kind, F, aligned, r)


@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "elementwise"])
@pytest.mark.parametrize("F", B.ATTENTION_WIDTHS)
def test_attention_grad_by_entries(F, aligned):
    from test_gpu_attention_grad_flat import T, run_flat
    for kind in ag_cases(F):
        g, _sg, _g1, dg = ag_inputs(kind)
        Wh, want, mag = ag_reference(kind, F)
        Whd = padded(Wh, aligned)
        got = run_flat(dg, g["capacity"], g["n_cols"], Whd, F)
        bound = FR.bound(g["rowptr"], T(), F, mag)
        r = ratio(got.double().cpu().numpy(), want, bound)
        print("attention_grad flat", kind, F, "vec" if aligned else "elementwise", f"worst error / bound {r:.3g}")
        assert torch.isfinite(got).all() and r <= 1.0, (kind, F, aligned, r)
