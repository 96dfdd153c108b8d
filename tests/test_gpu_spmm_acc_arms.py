"""Every arm of the two-pass aggregation sgx_spmm_csr_acc (csrc/spmm_csr.hip) against float64 (tests/_spmm_acc_ref.py).

The edges of a CSR are cut into two disjoint sets by column (col < n_cols / 2), so many rows are empty in one pass only and
some in both; pass 1 leaves fp32 partials, pass 2 starts from them.  Bounds (derived in _spmm_acc_ref.py, U = 2^-24):
an fp32 partial of a row of n terms is within (n + 2) U (|A| @ |H|) of float64 -- any summation order, so the split path
too; a stored result adds 2^-11 |want| + 2^-25 (fp16) or 2^-24 |want| (fp32); the second pass is checked against
float64(acc_in as the GPU produced it) + the float64 sum of pass 2 with scale |acc_in| + scale_2.  Dropping or doubling
one edge of a ten-edge row exceeds these bounds by three (fp16 result) to five (fp32 partial) orders of magnitude
(tests/test_spmm_acc_ref_cpu.py shows it).

Which arm a case takes: use_plan=False = the sblock path with CPL 1 at the lane split of P (scalar gathers where rows start on
odd halves, dword gathers on a dword-aligned pitch, 16-byte rows otherwise); SGX_SPMM_CPL forces CPL 1 / 2 / 4, a planned
adjacency of mean degree below 5 picks CPL 2 by itself; a plan with rows over 64 entries = the split path and
spmm_split_finalize_kernel; a degree-ordered plan with 4096 and more one-step rows = spmm_short_rows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _spmm_acc_ref as R

pytestmark = pytest.mark.gpu
TDT = {"f16": torch.float16, "f32": torch.float32}
SENTINEL = -77.0

GRAPHS, N_COLS = R.GRAPHS, R.N_COLS                      # shared with the CPU check of the restatement


@functools.lru_cache(maxsize=None)
def graph(name, dt):
    return GRAPHS[name](dt)


@functools.lru_cache(maxsize=None)
def csr(name, dt, which, planned):
    """the device matrix: A, A1 (pass 1), A2 (pass 2) or E (no edge at all); planned = its row schedule built and kept"""
    from sgracex1_amd import ops
    A = graph(name, dt)
    rp, ci, va = R.empty_like(A[0]) if which == "E" else A[("A", "A1", "A2").index(which)]
    M = ops.Csr(torch.as_tensor(rp, dtype=torch.int32, device="cuda"), torch.as_tensor(ci, dtype=torch.int32, device="cuda"),
                torch.as_tensor(va).to(TDT[dt]).cuda(), N_COLS[name])
    if planned and which != "E":
        assert M.plan.long_threshold == 64                   # under 2^20 entries every plan cuts at 64
        assert M.plan.long_rows == int((np.diff(rp) > 64).sum())
    return M


@functools.lru_cache(maxsize=6)
def ref(name, dt, P):
    """the table and the float64 sums / scales / term counts of A, A1 and A2, computed once"""
    A, A1, A2 = graph(name, dt)
    H = R.graph_table(name, P, dt)
    return dict(H=H, A=R.one_pass(A, H), A1=R.one_pass(A1, H), A2=R.one_pass(A2, H))


def table_dev(H, dt, pitch=None):
    """the table on the device; pitch: rows of that many elements, the columns beyond P filled with 9 (never to be read
    into a sum)"""
    t = torch.as_tensor(H).to(TDT[dt]).cuda()
    if pitch is None or pitch == H.shape[1]:
        return t.contiguous()
    buf = torch.full((H.shape[0], pitch), 9.0, dtype=TDT[dt], device="cuda")
    buf[:, :H.shape[1]] = t
    return buf[:, :H.shape[1]]


def _np(t):
    return t.double().cpu().numpy()


def check_passes(dt, r, mats, Ht, use_plan=True, tune=None):
    """Pass 1 -> fp32 partial, pass 2 -> D, with every property of the module docstring asserted.  Returns (partial, D)."""
    from sgracex1_amd import _lib, ops
    A, A1, A2, E = mats
    with _lib.tuning(**(tune or {})):
        part = ops.spmm_acc(A1, Ht, partial_out=True, use_plan=use_plan)
        D = ops.spmm_acc(A2, Ht, relu=True, acc_in=part, use_plan=use_plan)
        single = ops.spmm(A, Ht, relu=True, use_plan=use_plan)
        whole = ops.spmm_acc(A, Ht, partial_out=True, use_plan=use_plan)
        via_empty = ops.spmm_acc(E, Ht, relu=True, acc_in=whole)
        via_zero = ops.spmm_acc(A, Ht, relu=True, acc_in=torch.zeros_like(whole), use_plan=use_plan)
    assert part.dtype == torch.float32 and D.dtype == TDT[dt]
    (s1, scale1, n1), (s2, scale2, n2), (s, scale, n) = r["A1"], r["A2"], r["A"]
    R.assert_within("partial", _np(part), s1, R.partial_bound(n1, scale1))
    empty1 = torch.as_tensor(n1 == 0, device="cuda")
    empty2 = torch.as_tensor(n2 == 0, device="cuda")
    assert int(empty1.sum()) > 0 and int(empty2.sum()) > 0 and int((empty1 & empty2).sum()) > 0
    assert not part[empty1].any()                                              # exactly 0.0
    acc = _np(part)
    R.assert_within("D", _np(D), *R.finished(acc + s2, R.partial_bound(n2, np.abs(acc) + scale2), dt, True))
    assert torch.equal(D[empty2], torch.relu(part[empty2]).to(TDT[dt]))        # no edge in pass 2: exactly act(acc_in)
    assert not D[empty1 & empty2].any()
    R.assert_within("single pass", _np(single), *R.finished(s, R.partial_bound(n, scale), dt, True))
    assert torch.equal(via_empty, single), "partial of all of A, then a pass without edges"
    assert torch.equal(via_zero, single), "acc_in = 0 over all of A"
    return part, D


def _mats(name, dt, planned):
    return tuple(csr(name, dt, w, planned) for w in ("A", "A1", "A2", "E"))


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("P", [1, 2, 7, 8, 21, 24, 41, 64, 100, 128, 256, 520])
def test_lane_splits_and_store_paths(dt, P):
    """the sblock path, CPL 1, at every lane split: one element per lane where fp16 rows start on odd halves (P = 1, 7, 21,
    41), dword gathers on a dword-aligned pitch (fp16 P = 2, 100; fp32 P = 1, 7, 21, 41), 16-byte rows otherwise; P = 520
    walks the columns in two (fp16) and three (fp32) tiles"""
    r = ref("base", dt, P)
    # (use_plan=False: all of A has over 8192 entries and would build itself a plan otherwise)
    check_passes(dt, r, _mats("base", dt, False), table_dev(r["H"], dt), use_plan=False)


@pytest.mark.parametrize("dt,P,pitch", [("f16", 47, 50), ("f32", 7, 7), ("f16", 5, 5)])
def test_gather_forms(dt, P, pitch):
    """dword-aligned rows (a view of 47 of 50 halves; 7 fp32) and rows on odd halves (5 halves, unpadded: ops._gatherable
    keeps this small table as it is and the kernel gathers one element per lane)"""
    from sgracex1_amd import ops
    r = ref("base", dt, P)
    Ht = table_dev(r["H"], dt, pitch)
    assert ops._gatherable(Ht, P, 8000) is Ht and Ht.stride(0) == pitch
    assert (Ht.stride(0) * Ht.element_size()) % 4 == (2 if (dt, P) == ("f16", 5) else 0)
    for planned in (False, True):                                # the sblock path, then the planned matrices (rows 5..7 cut)
        check_passes(dt, r, _mats("base", dt, planned), Ht, use_plan=planned)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("P", [64, 256])
def test_cpl_1_2_4(dt, P):
    """forced lane-group sizes: the fma chain of an output element is the row's edges in order whatever the group, so rows
    the plan does not cut have the same bits under all three.  Then the same passes unforced on the planned second-pass
    adjacency, whose mean degree is below 5: choose_cpl takes 2 there (what a halo adjacency gets).  That run is checked
    like every other; which CPL it took is not observable from outside -- the premises (a plan, mean degree < 5) are
    asserted, the selection itself is not."""
    r = ref("base", dt, P)
    mats = _mats("base", dt, True)
    Ht = table_dev(r["H"], dt)
    uncut1 = torch.as_tensor(r["A1"][2] <= 64, device="cuda")
    uncut = uncut1 & torch.as_tensor(r["A2"][2] <= 64, device="cuda")
    assert int((~uncut1).sum()) == 2 and int((~uncut).sum()) == 3
    outs = {cpl: check_passes(dt, r, mats, Ht, tune={"SGX_SPMM_CPL": str(cpl)}) for cpl in (1, 2, 4)}
    for cpl in (2, 4):
        assert torch.equal(outs[cpl][0][uncut1], outs[1][0][uncut1]) and torch.equal(outs[cpl][1][uncut], outs[1][1][uncut])
    assert mats[2].nnz / mats[2].n_rows < 5.0 and mats[2]._plan is not None
    part, D = check_passes(dt, r, mats, Ht, tune={"SGX_SPMM_CPL": None})
    assert torch.equal(part[uncut1], outs[2][0][uncut1]) and torch.equal(D[uncut], outs[2][1][uncut])


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("P", [41, 64])
def test_split_path(dt, P):
    """rows of 65, 513 and 1 400 entries in pass 1 only, in pass 2 only and in both, through the plan's tasks and
    spmm_split_finalize_kernel (which starts from acc_in); then the same matrices without a plan"""
    r = ref("split", dt, P)
    mats = _mats("split", dt, True)
    assert [m.plan.long_rows for m in mats[:3]] == [9, 6, 6]
    Ht = table_dev(r["H"], dt)
    part, D = check_passes(dt, r, mats, Ht)
    part0, D0 = check_passes(dt, r, mats, Ht, use_plan=False)
    short1 = torch.as_tensor(r["A1"][2] <= 64, device="cuda")
    short = short1 & torch.as_tensor(r["A2"][2] <= 64, device="cuda")
    assert torch.equal(part[short1], part0[short1]) and torch.equal(D[short], D0[short])


@pytest.mark.parametrize("dt,P", [("f16", 64), ("f16", 100), ("f16", 128), ("f32", 32)])
def test_short_tail(dt, P):
    """a degree-ordered plan whose order ends in more than 4 096 one-step rows: spmm_short_rows loads acc_in and stores the
    partial or D for 64 rows per wavefront; both passes against float64 and, bit for bit, against the sblock walk of the
    same rows (SGX_SPMM_NO_SHORT_TAIL)"""
    r = ref("tail", dt, P)
    mats = _mats("tail", dt, True)
    for m, (_, _, n) in zip(mats[1:3], (r["A1"], r["A2"])):
        assert m.plan.reordered and m.plan.long_rows == 2
        assert int((n <= 8).sum()) >= 4096 and m.nnz / m.n_rows >= 5.0         # a tail, and CPL 1
    Ht = table_dev(r["H"], dt)
    part, D = check_passes(dt, r, mats, Ht)
    part0, D0 = check_passes(dt, r, mats, Ht, tune={"SGX_SPMM_NO_SHORT_TAIL": "1"})
    assert torch.equal(part, part0) and torch.equal(D, D0)
    # partial in AND out through the tail: rows without an edge in pass 2 (the end of its degree order) keep their sums
    from sgracex1_amd import _lib, ops
    (s2, scale2, n2) = r["A2"]
    both = ops.spmm_acc(mats[2], Ht, acc_in=part, partial_out=True)
    R.assert_within("partial to partial", _np(both), *R.second_pass(_np(part), graph("tail", dt)[2], r["H"]))
    empty2 = torch.as_tensor(n2 == 0, device="cuda")
    assert torch.equal(both[empty2], part[empty2]) and bool(part[empty2].any(1).sum() > 400)
    with _lib.tuning(SGX_SPMM_NO_SHORT_TAIL="1"):
        assert torch.equal(ops.spmm_acc(mats[2], Ht, acc_in=part, partial_out=True), both)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("P", [41, 64])
def test_partial_to_partial_chain(dt, P):
    """the edges cut three ways by column: partial -> partial (acc_in AND acc_out) -> result, each stage against float64 of
    the stage before as the GPU produced it"""
    from sgracex1_amd import ops
    A = graph("base", dt)[0]
    H = ref("base", dt, P)["H"]
    Ht = table_dev(H, dt)
    cuts = [A[1] < 267, (A[1] >= 267) & (A[1] < 533), A[1] >= 533]
    acc = None
    for k, m in enumerate(cuts):
        sub = R.subset(A, m)
        M = ops.Csr(torch.as_tensor(sub[0], device="cuda"), torch.as_tensor(sub[1], device="cuda"),
                    torch.as_tensor(sub[2]).to(TDT[dt]).cuda(), 800)
        M.plan
        prev = np.zeros((1000, P)) if acc is None else _np(acc)
        want, bound = R.second_pass(prev, sub, H)
        last = k == 2
        acc_new = ops.spmm_acc(M, Ht, relu=last, acc_in=acc, partial_out=not last)
        if last:
            want, bound = R.finished(want, bound, dt, True)
        R.assert_within(f"stage {k}", _np(acc_new), want, bound)
        none = torch.as_tensor(np.diff(sub[0]) == 0, device="cuda")
        if acc is not None and not last:
            assert torch.equal(acc_new[none], acc[none])                         # untouched rows pass through exactly
        acc = acc_new
    s, scale, n = ref("base", dt, P)["A"]
    # against the one float64 sum: stage k is off by (n_k + 2) U (|acc| + scale_k) <= (n_k + 2) U scale, three stages
    R.assert_within("chain vs one sum", _np(acc), *R.finished(s, R.partial_bound(n + 4, scale), dt, True))


def _acc_call(A, Ht, ldh, D, ldd, acc_in, acc_out, ld_acc, relu, plan):
    from sgracex1_amd import _lib, ops
    P = Ht.shape[1]
    sbytes = _lib.lib.sgx_spmm_scratch_bytes(plan.handle, P) if plan is not None else 0
    scratch = torch.empty(max(1, sbytes), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return _lib.lib.sgx_spmm_csr_acc(ops.dtype_code(Ht.dtype), int(relu), A.n_rows, Ht.shape[0], P, ptr(A.rowptr), ptr(A.col),
                                     ptr(A.val), ptr(Ht), ldh, ptr(D), ldd, ptr(acc_in), ptr(acc_out), ld_acc,
                                     plan.handle if plan is not None else None, ptr(scratch), sbytes,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("P", [41, 64])
def test_padded_partials_and_results(dt, P):
    """ld_acc = P + 3 and a D pitch of P + 5 through the C ABI, on the matrix with split-path rows and a short tail: the pad
    columns (and 64 guard rows behind the last row) keep their sentinel; the sums are those of the packed call"""
    from sgracex1_amd import ops
    r = ref("tail", dt, P)
    A, A1, A2, _ = _mats("tail", dt, True)
    n = A.n_rows
    Ht = table_dev(r["H"], dt)                              # fp16 P = 41: rows on odd halves, one element per lane
    ld_acc, ldd = P + 3, P + 5
    acc = torch.full((n + 64, ld_acc), SENTINEL, dtype=torch.float32, device="cuda")
    Dbuf = torch.full((n + 64, ldd), SENTINEL, dtype=TDT[dt], device="cuda")
    assert _acc_call(A1, Ht, Ht.stride(0), None, 0, None, acc, ld_acc, 0, A1.plan) == 0
    assert _acc_call(A2, Ht, Ht.stride(0), Dbuf, ldd, acc, None, ld_acc, 1, A2.plan) == 0
    assert (acc[:, P:] == SENTINEL).all() and (acc[n:] == SENTINEL).all()
    assert (Dbuf[:, P:] == SENTINEL).all() and (Dbuf[n:] == SENTINEL).all()
    (s1, scale1, n1), (s2, scale2, n2) = r["A1"], r["A2"]
    part = acc[:n, :P]
    R.assert_within("partial", _np(part), s1, R.partial_bound(n1, scale1))
    R.assert_within("D", _np(Dbuf[:n, :P]), *R.finished(_np(part) + s2, R.partial_bound(n2, np.abs(_np(part)) + scale2), dt, True))
    if ops._gatherable(Ht, P, A1.nnz) is Ht:                # the wrapper would gather from the same table: same chains
        packed = ops.spmm_acc(A1, Ht, partial_out=True)
        assert torch.equal(packed, part)
        assert torch.equal(ops.spmm_acc(A2, Ht, relu=True, acc_in=packed), Dbuf[:n, :P])


def test_rejections_touch_nothing():
    """D and acc_out both given, or ld_acc < n_feat: SGX_ERR_SHAPE before any launch"""
    dt, P = "f16", 64
    A1 = csr("base", dt, "A1", True)
    Ht = table_dev(ref("base", dt, P)["H"], dt)
    acc = torch.full((A1.n_rows, P), SENTINEL, dtype=torch.float32, device="cuda")
    acc_in = torch.full((A1.n_rows, P), 1.0, dtype=torch.float32, device="cuda")
    D = torch.full((A1.n_rows, P), SENTINEL, dtype=torch.float16, device="cuda")
    shape_err = -2                                           # SGX_ERR_SHAPE (include/sgx.h)
    assert _acc_call(A1, Ht, P, D, P, None, acc, P, 1, A1.plan) == shape_err
    assert _acc_call(A1, Ht, P, None, 0, None, acc, P - 1, 0, A1.plan) == shape_err
    assert _acc_call(A1, Ht, P, D, P, acc_in, None, P - 1, 1, A1.plan) == shape_err
    torch.cuda.synchronize()
    assert (acc == SENTINEL).all() and (D == SENTINEL).all() and (acc_in == 1.0).all()
