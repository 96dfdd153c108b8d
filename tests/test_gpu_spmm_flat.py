"""The entry-split aggregation sgx_spmm_csr_flat (csrc/spmm_flat.hip) against float64 on the smallest graphs at which its
ownership rule can fail (tests/_spmm_flat_ref.py: T = sgx_spmm_flat_chunk(); nnz in {0, 1, T - 1, T, T + 1}, a row of
5T + 3 entries leading and in the middle, a row ending on a chunk end followed by an empty row and a crossing one, empty rows
first, last and 70 of them at a chunk end, one row, a row that begins on a chunk's last entry, nnz passed as a capacity 3T
above the real count), at n_feat in {1, 3, 41, 64, 65, 256, 520}, fp16 and fp32, tables on 16-byte, dword and odd-half
pitches, D at pitch n_feat + 5 with sentinels in the pad columns and behind the last row, relu 0 and 1.

Bound (tests/_spmm_acc_ref.py, derived there, not tuned): an fp32 sum of n terms in ANY order -- the entry-order chain of
a lane group, the fold of the lane groups of a long piece, the chunk-order sum of a crossing row's partials -- is within
(n + 2) U |A| @ |H| of float64, U = 2^-24; the store adds 2^-11 |want| + 2^-25 (fp16) or 2^-24 |want| (fp32).  Dropping,
doubling or misplacing one entry of a ten-entry row moves a sum by ~0.25, three to five orders of magnitude outside.
Every case runs twice and must give equal bits.  Then: the recorded call replayed on another matrix inside the same
capacity, and ops.spmm without the fact and without schedule= bit for bit what sgx_spmm_csr gives with the same plan."""
import functools

import numpy as np
import pytest
import torch

import _spmm_acc_ref as R
import _spmm_flat_ref as F

pytestmark = pytest.mark.gpu
TDT = {"f16": torch.float16, "f32": torch.float32}
CODE = {"f16": 0, "f32": 1}
SENTINEL = -77.0
N_COLS = 97
WIDTHS = [1, 3, 41, 64, 65, 256, 520]


@functools.lru_cache(maxsize=None)
def T():
    from sgracex1_amd import _lib
    return _lib.lib.sgx_spmm_flat_chunk()


@functools.lru_cache(maxsize=None)
def graph(name, dt):
    deg, extra = F.degree_cases(T())[name]
    return F.build(deg, N_COLS, dt, seed=len(name)), extra


@functools.lru_cache(maxsize=None)
def graph_dev(name, dt):
    """(rowptr, col, val, capacity) on the device; col / val hold `capacity` entries, those behind the real end poisoned:
    a column far outside the table and a NaN, never to be read"""
    (rp, ci, va), extra = graph(name, dt)
    cap = len(ci) + extra
    col = torch.full((max(cap, 1),), 1 << 30, dtype=torch.int32, device="cuda")
    val = torch.full((max(cap, 1),), float("nan"), dtype=TDT[dt], device="cuda")
    col[:len(ci)] = torch.as_tensor(ci)
    val[:len(ci)] = torch.as_tensor(va).to(TDT[dt])
    return torch.as_tensor(rp, dtype=torch.int32, device="cuda"), col, val, cap


@functools.lru_cache(maxsize=4)
def table(P, dt):
    return R.table(np.random.default_rng(1000 + P), N_COLS, P, dt)


def table_dev(H, dt, pitch):
    """rows `pitch` elements apart, the columns beyond P filled with 9 (never to be read into a sum)"""
    buf = torch.full((H.shape[0], pitch), 9.0, dtype=TDT[dt], device="cuda")
    buf[:, :H.shape[1]] = torch.as_tensor(H).to(TDT[dt])
    return buf


def run_flat(dt, g, Ht, P, relu, ldd=None):
    """one call of the C entry point into a sentinel-filled D of pitch ldd with one row behind the last; returns all of it"""
    from sgracex1_amd import _lib, ops
    rp, col, val, cap = g
    n = rp.numel() - 1
    ldd = P + 5 if ldd is None else ldd
    D = torch.full((n + 1, ldd), SENTINEL, dtype=TDT[dt], device="cuda")
    sbytes = _lib.lib.sgx_spmm_flat_scratch_bytes(cap, P)
    assert sbytes > 0
    scratch = torch.full((sbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    ops.check(_lib.lib.sgx_spmm_csr_flat(CODE[dt], relu, n, Ht.shape[0], P, cap, rp.data_ptr(), col.data_ptr(), val.data_ptr(),
                                         Ht.data_ptr(), Ht.stride(0), D.data_ptr(), ldd, scratch.data_ptr(), sbytes,
                                         torch.cuda.current_stream().cuda_stream), "sgx_spmm_csr_flat")
    return D


def check_case(name, dt, P, pitch, relus=(0, 1)):
    (csr, _), g = graph(name, dt), graph_dev(name, dt)
    H = table(P, dt)
    Ht = table_dev(H, dt, pitch)
    s, scale, n_terms = R.one_pass(csr, H)
    n = len(csr[0]) - 1
    for relu in relus:
        D = run_flat(dt, g, Ht, P, relu)
        again = run_flat(dt, g, Ht, P, relu)
        assert torch.equal(D.view(torch.int16 if dt == "f16" else torch.int32), again.view(torch.int16 if dt == "f16" else torch.int32)), \
            f"{name} P={P} relu={relu}: two runs differ"
        got = D.double().cpu().numpy()
        assert (got[:n, P:] == SENTINEL).all() and (got[n] == SENTINEL).all(), f"{name} P={P}: a store outside the rows of D"
        want, bound = R.finished(s, R.partial_bound(n_terms, scale), dt, relu)
        R.assert_within(f"{name} {dt} P={P} pitch={pitch} relu={relu}", got[:n, :P], want, bound)
        empty = n_terms == 0
        if empty.any():                                  # act(0) = +0, bit for bit
            assert not D[:n, :P][torch.as_tensor(empty, device="cuda")].view(torch.int16 if dt == "f16" else torch.int32).any(), name


def pitch_16(P, dt):
    per16 = 8 if dt == "f16" else 4
    return -(-P // per16) * per16


@pytest.mark.parametrize("P", WIDTHS)
@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_rule_on_every_graph(dt, P):
    """rows of the table on 16 bytes: 16-byte gathers"""
    for name in F.degree_cases(T()):
        check_case(name, dt, P, pitch_16(P, dt))


@pytest.mark.parametrize("P,pitch", [(1, 1), (3, 3), (41, 41), (65, 65), (41, 43), (520, 521)])
def test_fp16_table_on_an_odd_half_pitch(P, pitch):
    """rows that start on odd halves: one element per lane"""
    for name in ("nnz_T+1", "long_middle", "ends_on_chunk_end", "empty_run", "begins_on_last_entry", "capacity", "mixed"):
        check_case(name, "f16", P, pitch)


@pytest.mark.parametrize("dt,P,pitch", [("f16", 41, 42), ("f16", 65, 66), ("f16", 3, 6), ("f32", 41, 41), ("f32", 65, 67), ("f32", 3, 3)])
def test_table_on_a_dword_pitch(dt, P, pitch):
    """rows that start on a dword but not on 16 bytes: 16-byte gathers that run into the next row, never stored"""
    for name in ("nnz_T+1", "long_leading", "ends_on_chunk_end", "one_row_long", "capacity", "mixed"):
        check_case(name, dt, P, pitch)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("P", [1, 8, 64, 520])
def test_sums_that_cancel_store_plus_zero(dt, P):
    """Pairs (+a, -a) on equal rows of H cancel exactly in every partial sum, and (-1) x 0 is -0 added to +0: a sum starts
    from +0 and so can never be -0, whatever the path -- a short row, a piece shared by all lane groups, a crossing row's
    partials -- and with and without the ReLU."""
    t = T()
    deg = [4, 2 * t + 10, 6, 70, 3]                                     # every row starts on an even entry
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    rng = np.random.default_rng(5)
    nnz = int(rp[-1])
    ci = rng.integers(0, 40, nnz).astype(np.int32)
    ci[1::2] = ci[0::2][:nnz // 2] + 40                                  # the pair's second column: an equal row of H
    # (values and table on the fp16 grid for fp32 too: an fp32 product of two of them is exact, so a pair cancels exactly)
    va = R.rounded(rng.random(nnz) + 0.25, "f16")
    va[1::2] = -va[0::2][:nnz // 2]
    ci[rp[4]:rp[5]], va[rp[4]:rp[5]] = 96, -1.0                          # row 4: three times (-1) x 0
    H = R.table(rng, N_COLS, P, "f16")
    H[40:80], H[96] = H[0:40], 0.0
    g = (torch.as_tensor(rp, device="cuda"), torch.as_tensor(ci, device="cuda"), torch.as_tensor(va).to(TDT[dt]).cuda(), nnz)
    Ht = table_dev(H, dt, pitch_16(P, dt))
    for relu in (0, 1):
        D = run_flat(dt, g, Ht, P, relu)
        assert not D[:len(deg), :P].view(torch.int16 if dt == "f16" else torch.int32).any(), (dt, P, relu)


def test_tiny_negative_sum_under_relu_is_plus_zero():
    """an fp32 sum that rounds to fp16 -0.0: the ReLU stores +0 (keep when v > 0, else +0), without it the rounded -0.0"""
    rp = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    g = (rp, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.tensor([-2.0 ** -14], dtype=torch.float16, device="cuda"), 1)
    Ht = torch.full((1, 8), 2.0 ** -14, dtype=torch.float16, device="cuda")
    assert (run_flat("f16", g, Ht, 8, 1)[:1, :8].view(torch.int16) == 0).all()
    assert (run_flat("f16", g, Ht, 8, 0)[:1, :8].view(torch.int16) == -32768).all()


# ---- ops.spmm: the keyword, the fact, the replay ---------------------------------------------------------------------------

def _csr(rp, ci, va, dt, capacity=None):
    from sgracex1_amd import ops
    cap = len(ci) if capacity is None else capacity
    col = torch.zeros(cap, dtype=torch.int32, device="cuda")
    val = torch.zeros(cap, dtype=TDT[dt], device="cuda")
    col[:len(ci)], val[:len(ci)] = torch.as_tensor(ci), torch.as_tensor(va).to(TDT[dt])
    return ops.Csr(torch.as_tensor(rp, dtype=torch.int32, device="cuda"), col, val, N_COLS)


def _replay_graph(seed, n_rows, long_row, long_len, mean):
    rng = np.random.default_rng(seed)
    deg = rng.poisson(mean, n_rows)
    deg[long_row] = long_len
    return F.build(deg, N_COLS, "f16", seed=seed)


def test_keyword_and_fact_take_the_flat_form():
    from sgracex1_amd import ops
    (rp, ci, va), _ = graph("mixed", "f16")
    H = torch.as_tensor(table(64, "f16")).half().cuda()
    A = _csr(rp, ci, va, "f16")
    by_keyword = ops.spmm(A, H, relu=True, schedule="flat")
    direct = run_flat("f16", graph_dev("mixed", "f16"), H, 64, 1, ldd=64)[:-1]
    assert torch.equal(by_keyword.view(torch.int16), direct.view(torch.int16))
    B = _csr(rp, ci, va, "f16").with_facts(flat=True)
    assert not B.wants_plan and B._plan is None
    assert torch.equal(ops.spmm(B, H, relu=True).view(torch.int16), direct.view(torch.int16))
    assert B._plan is None                                              # no plan was built on the way
    C = B.to(torch.float32)
    assert C._flat and not C.wants_plan and C._plan is None
    s, scale, n_terms = R.one_pass((rp, ci, va), table(64, "f16"))
    want, bound = R.finished(s, R.partial_bound(n_terms, scale), "f32", 0)
    R.assert_within("fact carried by to()", ops.spmm(C, H.float()).double().cpu().numpy(), want, bound)


def test_recorded_call_replays_on_another_matrix():
    """~10 000 entries with a row of 2000, recorded with the fact under sync-debug "error"; then rowptr, col and val are
    overwritten in place with a matrix of another degree profile and fewer entries: the replay equals an eager call on it."""
    from sgracex1_amd import ops
    n_rows = 1300
    first = _replay_graph(1, n_rows, 17, 2000, 6.2)
    second = _replay_graph(2, n_rows, 900, 1500, 4.0)
    cap = len(first[1])
    assert 9000 <= cap <= 11000 and len(second[1]) < cap - T()
    A = _csr(*first, "f16", capacity=cap).with_facts(flat=True)
    H = torch.as_tensor(table(64, "f16")).half().cuda()
    out = torch.empty((n_rows, 64), dtype=torch.float16, device="cuda")
    ops.spmm(A, H, relu=True, out=out)                                   # sizes the workspace outside the recording
    eager_first = out.clone()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.graph(graph_):
            ops.spmm(A, H, relu=True, out=out, schedule="flat")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert A._plan is None
    out.fill_(SENTINEL)
    graph_.replay()
    assert torch.equal(out.view(torch.int16), eager_first.view(torch.int16))
    rp2, ci2, va2 = second
    A.rowptr.copy_(torch.as_tensor(rp2, dtype=torch.int32))
    A.col[:len(ci2)] = torch.as_tensor(ci2).cuda()
    A.col[len(ci2):] = 1 << 30                                           # what lies behind the new end is never read
    A.val[:len(ci2)] = torch.as_tensor(va2).half().cuda()
    A.val[len(ci2):] = float("nan")
    out.fill_(SENTINEL)
    graph_.replay()
    replayed = out.clone()
    eager = ops.spmm(_csr(rp2, ci2, va2, "f16", capacity=cap), H, relu=True, schedule="flat")
    assert torch.equal(replayed.view(torch.int16), eager.view(torch.int16))
    s, scale, n_terms = R.one_pass(second, table(64, "f16"))
    want, bound = R.finished(s, R.partial_bound(n_terms, scale), "f16", 1)
    R.assert_within("replay on the second matrix", replayed.double().cpu().numpy(), want, bound)


@pytest.mark.parametrize("planned", [True, False])
def test_default_call_is_unchanged(planned):
    """without the fact and without schedule=: the bits of sgx_spmm_csr with the plan ops.spmm picks (a row over 64 entries
    in a matrix of 8192 and more entries wants one; a small matrix wants none)"""
    from sgracex1_amd import _lib, ops
    rng = np.random.default_rng(11)
    deg = rng.poisson(9.0, 1000) if planned else rng.poisson(5.0, 300)
    if planned:
        deg[5], deg[700] = 300, 90
    rp, ci, va = F.build(deg, N_COLS, "f16", seed=3)
    A = _csr(rp, ci, va, "f16")
    assert A.wants_plan == planned and (A.nnz >= 8192) == planned and not A._flat
    H = torch.as_tensor(table(64, "f16")).half().cuda()
    got = ops.spmm(A, H, relu=True)
    assert (A._plan is not None) == planned
    if planned:
        assert A.plan.long_rows == 2
    plan = A.plan.handle if planned else None
    sbytes = _lib.lib.sgx_spmm_scratch_bytes(plan, 64) if planned else 0
    scratch = torch.empty(max(sbytes, 256), dtype=torch.uint8, device="cuda")
    D = torch.full((len(deg), 64), SENTINEL, dtype=torch.float16, device="cuda")
    ops.check(_lib.lib.sgx_spmm_csr(0, _lib.SGX_ACC_F32, 1, 1, len(deg), N_COLS, 64, A.rowptr.data_ptr(), A.col.data_ptr(),
                                    A.val.data_ptr(), H.data_ptr(), 64, D.data_ptr(), 64, plan, scratch.data_ptr(), sbytes,
                                    torch.cuda.current_stream().cuda_stream), "sgx_spmm_csr")
    assert torch.equal(got.view(torch.int16), D.view(torch.int16))
    flat = ops.spmm(A, H, relu=True, schedule="flat")                     # and the flat form agrees within the bound
    s, scale, n_terms = R.one_pass((rp, ci, va), table(64, "f16"))
    want, bound = R.finished(s, R.partial_bound(n_terms, scale), "f16", 1)
    R.assert_within("flat beside the default", flat.double().cpu().numpy(), want, bound)
    if not planned:                                                       # rows inside one chunk: the unplanned call's bits
        inside = torch.as_tensor(rp[:-1] // T() == (np.maximum(rp[1:], 1) - 1) // T(), device="cuda")
        assert torch.equal(flat[inside].view(torch.int16), got[inside].view(torch.int16))
