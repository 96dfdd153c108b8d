"""SGX_ACC_REF_HALF on every kernel arm of csrc/refhalf.hip, bit for bit against tests/_refhalf_ref.py (numpy float16, held
to the oracle's model by tests/test_refhalf_ref_cpu.py), with oracle.layer_refhalf as a second witness where the entry point
is the whole layer.  tests/test_gpu_refhalf.py runs the mode on the reference's matrices; the arm a call takes depends on the
output width, the table's alignment and the row count alone, and each case here builds the shape that selects one arm -- the
rule is restated beside the case.  Every comparison is np.array_equal on the uint16 bit patterns; there is no tolerance.

The inputs (tests/_refhalf_ref.py): a 598-row graph with row lengths 0..5, 31..33, 63..65 and 300, two empty rows in one
sblock and every phase under spmm_block 2, 3, 4; five hostile rows behind it -- a partial that overflows to +inf, inf - inf
in the fold, products that are all -0 (the sum is +0), a positive subnormal sum and a negative one; dense inputs with 30 %
zeros and an overflowing and a NaN row."""
import functools

import numpy as np
import pytest
import torch

import _refhalf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def _csr(triple, n_cols):
    from sgracex1_amd import ops
    rp, ci, va = triple
    return ops.Csr(_dev(rp.astype(np.int32)), _dev(ci.astype(np.int32)), _dev(np.asarray(va, np.float16)), n_cols)


def _host(t):
    return t.cpu().numpy()


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float16), np.asarray(want, np.float16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = R.bits(got), R.bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ in {len(set(bad[:, 0]))} rows and "
                             f"{len(set(bad[:, 1]))} columns; first at {i}: got 0x{g[i]:04x}, want 0x{w[i]:04x}")


@functools.lru_cache(maxsize=None)
def _graph():
    return R.hostile_graph()


@functools.lru_cache(maxsize=None)
def _want_ah(P, spmm_block, relu):
    g, _ = _graph()
    out = R.csr_stage(*g, R.table(P), spmm_block, 1, relu)
    out.setflags(write=False)
    return out


def _table_on_device(T, pitch, offset=0):
    """T in columns [offset, offset + P) of a [rows, pitch] buffer whose other columns hold 1234 (never to be seen)."""
    buf = torch.full((T.shape[0], pitch), 1234.0, dtype=torch.float16, device=DEV)
    view = buf[:, offset:offset + T.shape[1]]
    view.copy_(_dev(T))
    return view


def _spmm_exact(A, Td, relu, spmm_block, out=None):
    from sgracex1_amd import ops
    return ops.spmm(A, Td, relu=bool(relu), acc_mode=ops.SGX_ACC_REF_HALF, spmm_block=spmm_block, out=out)


# (a) refhalf_csr_rows_kernel<LPR>: taken when the table pointer and its pitch in bytes are multiples of 16;
# LPR = clamp(next_pow2(ceil(P / 8)), 4, 64) lanes own a row, 8 columns each; P > 8 * LPR walks column tiles of 512.
#   P  21 (pitch 24)  LPR 4, the last lane stores 5 single elements
#   P  24             LPR 4        P 40   LPR 8        P 64, 100  LPR 8, 16 (100: the last lane holds 4 columns)
#   P 129             LPR 32, lane 16 holds one column          P 256  LPR 32
#   P 300, 512        LPR 64       P 520  LPR 64, a second column tile of 8 columns       P 1000  LPR 64, two tiles
# The pitch is the width rounded up to 8 halves (the smallest aligned one; 16 more for P = 256 and 512, which are aligned
# as they are), so 16-byte gathers at a ragged end read the pad columns.
_AH_ROWS = {21: 24, 24: 24, 40: 40, 64: 64, 100: 104, 129: 136, 256: 272, 300: 304, 512: 528, 520: 520, 1000: 1000}


@pytest.mark.parametrize("P", sorted(_AH_ROWS))
def test_csr_stage_lane_group_arms(P):
    g, rows = _graph()
    A = _csr(g, R.N_COLS)
    Td = _table_on_device(R.table(P), _AH_ROWS[P])
    assert Td.data_ptr() % 16 == 0 and (Td.stride(0) * 2) % 16 == 0                     # what selects the lane-group form
    for spmm_block in R.AH_BLOCKS:
        for relu in (0, 1):
            got = _host(_spmm_exact(A, Td, relu, spmm_block))
            assert_bits(got, _want_ah(P, spmm_block, relu), f"P {P} spmm_block {spmm_block} relu {relu}")
    raw = _want_ah(P, 4, 0)
    assert np.isposinf(raw[rows["inf"]]).all() and np.isnan(raw[rows["nan"]]).all() and (R.bits(raw[rows["negzero"]]) == 0).all()
    # a pitched result: the columns behind P keep what they held
    pad = 5
    buf = torch.full((A.n_rows, P + pad), -77.0, dtype=torch.float16, device=DEV)
    got = _spmm_exact(A, Td, 1, 3, out=buf[:, :P])
    assert got.data_ptr() == buf.data_ptr()
    assert_bits(_host(buf[:, :P]), _want_ah(P, 3, 1), f"P {P} pitched out")
    assert bool((buf[:, P:] == -77.0).all())


# (b) refhalf_csr_kernel, one thread per output: taken when the table pointer or its pitch is not a multiple of 16 bytes.
#   P 41 contiguous: pitch 82 bytes.      P 64 as columns 4..67 of a buffer of pitch 72: the pitch is 144 bytes, the
#   pointer 8 bytes off -- the same values as (a)'s P = 64, so the two arms are also held to each other.
def test_csr_stage_scalar_arm():
    g, _ = _graph()
    A = _csr(g, R.N_COLS)
    odd = _dev(R.table(41))
    assert (odd.stride(0) * 2) % 16 != 0
    shifted = _table_on_device(R.table(64), 72, offset=4)
    assert (shifted.stride(0) * 2) % 16 == 0 and shifted.data_ptr() % 16 == 8
    aligned = _table_on_device(R.table(64), 64)
    for spmm_block in R.AH_BLOCKS:
        for relu in (0, 1):
            assert_bits(_host(_spmm_exact(A, odd, relu, spmm_block)), _want_ah(41, spmm_block, relu), f"P 41 {spmm_block} {relu}")
            scalar = _host(_spmm_exact(A, shifted, relu, spmm_block))
            lanes = _host(_spmm_exact(A, aligned, relu, spmm_block))
            assert_bits(scalar, lanes, f"scalar arm against lane-group arm, {spmm_block} {relu}")
            assert_bits(scalar, _want_ah(64, spmm_block, relu), f"P 64 shifted {spmm_block} {relu}")


# (c) the dense stage.  refhalf_dense_rows_kernel<LPR> for n >= 1024 and P <= 512, LPR = next_pow2(ceil(P / 8)) (1, 2, 4, 8
# and 32 run in test_gpu_refhalf.py); a block of kc_rows = min(128, 64 KB / (16 LPR bytes)) weight rows sits in LDS.
#   1100 x  70 -> 100   LPR 16, one k-block; phases 0 and 2          1100 x 71 -> 100   LPR 16, every phase
#   1100 x 130 -> 300   LPR 64: kc_rows 64, k-blocks of 64, 64 and 2  1100 x 67 -> 300   LPR 64, two k-blocks, every phase
#   1100 x  40 -> 300   LPR 64, one k-block
#   8215 x  40 -> 300   LPR 64, 4 rows per workgroup: 2054 row groups > 2048, so W is staged once and the workgroups
#                       walk the groups in a stride; the last group holds 3 rows
# refhalf_dense_kernel, one thread per output, otherwise:
#   1100 x  33 -> 600   P > 512                                       1000 x 33 -> 100   fewer than 1024 rows
@pytest.mark.parametrize("n,M,P", R.DENSE_CASES)
def test_dense_stage_arms(n, M, P):
    from sgracex1_amd import ops
    x, wt = R.dense_case(n, M, P)
    X, Wt = _dev(x), _dev(wt)
    for spmm_block in R.DENSE_BLOCKS:
        want = R.dense_stage(x, wt, spmm_block)
        got = ops.xw_dense(X, Wt, acc_mode=ops.SGX_ACC_REF_HALF, spmm_block=spmm_block)     # the gather pitch, > P here
        full = got._base
        assert full.shape[1] > P and got.stride(0) == full.shape[1]
        assert_bits(_host(got), want, f"{n}x{M}->{P} spmm_block {spmm_block}")
        assert bool((full[:, P:].view(torch.int16) == 0).all())                               # pad columns: +0 exactly
        tight = ops.xw_dense(X, Wt, ldh=P, acc_mode=ops.SGX_ACC_REF_HALF, spmm_block=spmm_block)
        assert_bits(_host(tight), want, f"{n}x{M}->{P} spmm_block {spmm_block}, ldh = P")
    assert np.isposinf(want[R.DENSE_INF_ROW]).all() and np.isnan(want[R.DENSE_NAN_ROW]).all()


# (d) thread splits that leave a remainder (sblock_first_row's clamp), fewer rows than threads (blk == 0), and the dense
# stage with threads: layer.hip calls sgx_refhalf_dense itself when fea_threads > 1 -- lane-group kernel at 1101 rows,
# one-thread-per-output kernel at 1023.  Sparse features 64 -> 129: both stages refhalf_csr_rows_kernel (LPR 32).
# M = 40 keeps every dense phase 0 (the split shows in A.H alone); M = 41 moves the dense phases as well.
@pytest.mark.parametrize("n,M,P,sparse,spmm_block,fea_threads,adj_threads", R.LAYER_CASES)
def test_layer_thread_splits_with_remainders(oracle, n, M, P, sparse, spmm_block, fea_threads, adj_threads):
    from sgracex1_amd import ops
    adj, fea, wt = R.layer_case(n, M, P, sparse)
    A = _csr(adj, n)
    X = _csr(fea, M) if sparse else _dev(fea)
    kw = dict(spmm_block=spmm_block, fea_threads=fea_threads, adj_threads=adj_threads)
    for relu in (0, 1):
        want, _ = R.layer(adj, fea, wt, relu, **kw)
        witness = oracle.layer_refhalf(0 if sparse else 1, relu, adj, fea, wt, **kw)
        got = _host(ops.layer_forward(A, X, _dev(wt), relu=bool(relu), acc_mode=ops.SGX_ACC_REF_HALF, **kw))
        assert_bits(got, want, f"layer {n} {M}->{P} {kw} relu {relu}")
        assert_bits(got, witness, f"layer {n} {M}->{P} {kw} relu {relu}, oracle")
    if n == 1101:                                                # the split is observable
        one, _ = R.layer(adj, fea, wt, 1, spmm_block)
        assert int((R.bits(one) != R.bits(want)).sum()) > 1000


# (e) the mode is on: against the default fp32-accumulate result of the same call, and each repeatable
def test_exact_mode_differs_from_default_and_repeats():
    from sgracex1_amd import ops
    g = R.adj_graph()
    A = _csr(g, R.N_COLS)
    Td = _table_on_device(R.table(256), 272)
    exact = _host(_spmm_exact(A, Td, 1, 4))
    fast = _host(ops.spmm(A, Td, relu=True))
    assert_bits(exact, R.csr_stage(*g, R.table(256), 4, 1, True), "ordinary rows alone")
    assert float((R.bits(exact) != R.bits(fast)).mean()) > 0.10
    assert np.array_equal(R.bits(exact), R.bits(_host(_spmm_exact(A, Td, 1, 4))))
    assert np.array_equal(R.bits(fast), R.bits(_host(ops.spmm(A, Td, relu=True))))
