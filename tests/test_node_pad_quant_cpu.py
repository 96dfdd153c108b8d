"""Padded quantised node batches without a GPU (include/sgx.h, sgx_node_batch_sample_padded_quant): the numpy restatement
(tests/_node_pad_quant_ref.py) on a hand-written batch, the two conditions the filler rows put on the quantiser constants
for the published constants of every width, the new symbol and every argument error before a device is touched, and what
NeighborLoader(pad=True, quant=) checks before any device work."""
import ctypes
import subprocess
from dataclasses import replace

import numpy as np
import pytest
import torch

import _node_pad_quant_ref as PQ

OK, NULL, SHAPE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_restated_padding_of_a_tiny_quantised_batch():
    """n = 2 live rows with a = 3 entries in a capacity of N = 5 rows and C_a = 70 entries (the batch of
    test_node_pad_cpu.py): 64 spare entries, 63 to filler row 0 and 1 to filler row 1.  inv_scale 3, zero 0, 2 bits: the
    grid is round(3 x) clipped to 0 .. 3, over 2."""
    cap = dict(N=5, Ca=70)
    rowptr = np.asarray([0, 2, 3], np.int32)
    val = np.asarray([0.5, 0.1, 1.0], np.float32)
    assert PQ.fq(val, 3, 0, 2).tolist() == [1.0, 0.0, 1.5]               # round(1.5) = 2 (half to even), round(0.3) = 0, 3
    assert PQ.fq([1, 0], 3, 0, 2).tolist() == [1.5, 0.0]
    q, dead, lean = PQ.live_quant(2, rowptr, val, 3, 0, 2)
    assert q.tolist() == [1.0, 0.0, 1.5] and dead.tolist() == [False, False] and lean.tolist() == q.tolist()
    out = PQ.pad_quant(cap, 2, rowptr, val, q, dead, lean, 3, 0, 2)
    assert out["values_q"].dtype == np.float32 and out["values_q"].shape == (70,)
    assert out["values_q"].tolist() == [1.0, 0.0, 1.5] + [1.5] + [0.0] * 63 + [1.5, 0.0] + [1.5]
    assert out["dead_row_q"].tolist() == [False] * 5
    assert out["values_lean"].tolist() == out["values_q"].tolist()
    # a live row that dies on the grid keeps its unquantised values in the lean form; the filler rows do not die
    q, dead, lean = PQ.live_quant(2, rowptr, np.asarray([0.1, 0.1, 1.0], np.float32), 3, 0, 2)
    assert dead.tolist() == [True, False] and lean.tolist() == [np.float32(0.1), np.float32(0.1), 1.5]
    out = PQ.pad_quant(cap, 2, rowptr, np.asarray([0.1, 0.1, 1.0], np.float32), q, dead, lean, 3, 0, 2)
    assert out["dead_row_q"].tolist() == [True, False, False, False, False]
    assert out["values_lean"][:3].tolist() == lean.tolist() and out["values_lean"][3:].tolist() == out["values_q"][3:].tolist()
    # constants the call refuses (a 1 that rounds to 0): by the rule the filler rows would be dead and their lean values 1, 0
    bad = PQ.pad_quant(cap, 2, rowptr, val, *PQ.live_quant(2, rowptr, val, 0.4, 0, 8), 0.4, 0, 8)
    assert bad["dead_row_q"][2:].all() and bad["values_lean"][3:5].tolist() == [1.0, 0.0]
    # the 1-bit grid: q / 2
    assert PQ.fq([1, 0.04, 0.06, 0], 10, 0, 1).tolist() == [0.5, 0.0, 0.5, 0.0]


@pytest.mark.parametrize("bits,rounded", [(8, 255), (4, 15), (2, 30), (1, 10)])
def test_filler_rows_are_live_and_weightless_for_the_published_constants(bits, rounded):
    """No filler row is dead (fq(1) > 0) and no spare entry carries weight (fq(0) == 0) for quant.constants(w): a_z = 0 and
    round(1 / a_s) is 255, 15, 30, 10 before the clip -- for both layers' constants, by the restatement, by
    sgrace._fq_unsigned and by the loader's own check."""
    from sgracex1_amd import pyg_lite, quant, sgrace
    qc = quant.constants(bits)
    for c in (qc, qc.second_layer()):
        inv, zero, q = PQ.constants_of(c)
        assert zero == 0 and int(np.rint(inv)) == rounded
        one, nought = PQ.fq([1.0], inv, zero, q)[0], PQ.fq([0.0], inv, zero, q)[0]
        assert one > 0 and nought == 0
        assert one == (0.5 if bits == 1 else (2 ** bits - 1) / 2 ** (bits - 1))          # the top of the grid
        t = sgrace._fq_unsigned(torch.tensor([1.0, 0.0]), c.a_s, c.a_z, c.w_qbits)
        assert t.tolist() == [float(one), 0.0]
        assert pyg_lite._fq_unsigned_scalar(1.0, c.a_s, c.a_z, bits) == float(one)
        assert pyg_lite._fq_unsigned_scalar(0.0, c.a_s, c.a_z, bits) == 0.0
    pyg_lite.check_pad_quant(qc)


def _valid_arguments(L):
    """(batch, pad, quant) structs that pass every argument check of the padded quantised call, with made-up addresses:
    changed one field at a time below, so nothing ever reaches a launch."""
    fan = (ctypes.c_int32 * 2)(10, 10)
    p = L.NodeBatchPad()
    assert L.lib.sgx_node_batch_pad_capacity(3000, 50000, 128, 2, fan, None, ctypes.byref(p)) == OK
    p.step = p.status = p.counts = 256
    d = L.NodeBatch()
    d.fanouts = fan
    d.n_nodes, d.nnz, d.batch, d.n_hops, d.dtype = 3000, 50000, 128, 2, 1          # SGX_F32
    mn, me = ctypes.c_int64(0), ctypes.c_int64(0)
    nbytes = L.lib.sgx_node_batch_workspace_bytes(3000, 50000, 128, 2, fan, ctypes.byref(mn), ctypes.byref(me))
    d.max_nodes, d.max_edges = mn.value, me.value
    for name in ("rowPtr", "columnIndex", "seeds", "node_map", "n_id", "out_rowPtr", "out_col", "edge_pos", "rowPtr_norm",
                 "columnIndex_norm", "values_norm", "dead_row"):
        setattr(d, name, 256)
    d.workspace, d.workspace_bytes = 256, nbytes
    q = L.NodeBatchQuant()
    q.n_sets, q.qbits = 2, 8
    for k in range(2):
        q.inv_scale_adj[k], q.zero_adj[k] = 255.0, 0.0
        q.values_q[k] = q.dead_row_q[k] = 256
    return d, p, q, fan, nbytes


def test_new_symbol_and_argument_errors_before_a_device_is_touched(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    name = "sgx_node_batch_sample_padded_quant"
    assert name in L.SYMBOLS and f" T {name}\n" in out
    assert L.lib.sgx_version() == 110
    call = L.lib.sgx_node_batch_sample_padded_quant
    d, p, q, fan, nbytes = _valid_arguments(L)
    B, P, Q = ctypes.byref(d), ctypes.byref(p), ctypes.byref(q)
    assert call(None, P, Q, None) == NULL and call(B, None, Q, None) == NULL and call(B, P, None, None) == NULL

    def with_field(struct, field, value, index=None):
        c = type(struct).from_buffer_copy(struct)
        if index is None:
            setattr(c, field, value)
        else:
            getattr(c, field)[index] = value
        return c

    # those of sgx_node_batch_sample_quant
    assert call(ctypes.byref(with_field(d, "dtype", 0)), P, Q, None) == UNSUPPORTED            # SGX_F16
    for n_sets in (0, 3, -1):
        assert call(B, P, ctypes.byref(with_field(q, "n_sets", n_sets)), None) == SHAPE
    for bits in (0, 3, 16, 32):
        assert call(B, P, ctypes.byref(with_field(q, "qbits", bits)), None) == SHAPE
    for field in ("values_q", "dead_row_q"):
        for k in (0, 1):
            assert call(B, P, ctypes.byref(with_field(q, field, None, k)), None) == NULL, (field, k)
    one_set = with_field(q, "n_sets", 1)
    one_set.values_q[1] = one_set.dead_row_q[1] = None                                          # set 1 is not looked at
    # the filler rows would be dead (1 rounds to 0) or would carry weight (0 does not stay 0), in either set
    for k in (0, 1):
        assert call(B, P, ctypes.byref(with_field(q, "inv_scale_adj", 0.4, k)), None) == UNSUPPORTED, k
        assert call(B, P, ctypes.byref(with_field(q, "zero_adj", 1.0, k)), None) == UNSUPPORTED, k
        assert call(B, P, ctypes.byref(with_field(q, "inv_scale_adj", float("nan"), k)), None) == UNSUPPORTED, k
        assert call(B, P, ctypes.byref(with_field(q, "inv_scale_adj", -255.0, k)), None) == UNSUPPORTED, k
    assert call(B, P, ctypes.byref(with_field(one_set, "inv_scale_adj", 0.4, 0)), None) == UNSUPPORTED
    assert call(B, P, ctypes.byref(with_field(with_field(q, "qbits", 1), "inv_scale_adj", 0.4, 0)), None) == UNSUPPORTED
    # those of the padded call, reached with valid quantiser arguments (one and two sets)
    for qq in (Q, ctypes.byref(with_field(one_set, "inv_scale_adj", 255.0, 0))):
        assert call(ctypes.byref(with_field(d, "fanouts", None)), P, qq, None) == NULL
        assert call(ctypes.byref(with_field(d, "batch", 0)), P, qq, None) == SHAPE
        assert call(ctypes.byref(with_field(d, "max_nodes", d.max_nodes - 1)), P, qq, None) == SHAPE
        for name in ("rowPtr", "seeds", "node_map", "values_norm", "dead_row"):
            assert call(ctypes.byref(with_field(d, name, None)), P, qq, None) == NULL, name
        assert call(ctypes.byref(with_field(d, "workspace_bytes", nbytes - 1)), P, qq, None) == WORKSPACE
        for name in ("step", "status", "counts"):
            assert call(B, ctypes.byref(with_field(p, name, None)), qq, None) == NULL, name
        mn, me = d.max_nodes, d.max_edges
        for field, value in (("n_rows", mn - 1), ("n_edges", me - 1), ("nnz_norm", me + p.n_rows - 1),
                             ("nnz_norm", p.n_rows + 63 * (p.n_rows - mn) + 1), ("nnz_norm", 1 << 31)):
            assert call(B, ctypes.byref(with_field(p, field, value)), qq, None) == SHAPE, field
        unbounded = with_field(d, "fanouts", (ctypes.c_int32 * 2)(10, -1))
        assert call(ctypes.byref(unbounded), P, qq, None) == UNSUPPORTED
    # the unquantised padded call takes the same arguments as before
    assert L.lib.sgx_node_batch_sample_padded(ctypes.byref(with_field(d, "batch", 0)), P, None) == SHAPE


def test_neighbor_loader_checks_the_constants_before_any_device_work():
    from sgracex1_amd import pyg_lite, quant
    data = pyg_lite.NodeData(torch.zeros((4, 3)), torch.zeros((2, 0), dtype=torch.int64))          # on the host
    kw = dict(batch_size=2, prepare="sym_norm2", pad=True)
    with pytest.raises(ValueError, match="quant"):
        pyg_lite.NeighborLoader(data, [3, 2], quant=quant.constants(8, a_s=4.0), **kw)               # 1 rounds to 0
    with pytest.raises(ValueError, match="quant"):
        pyg_lite.NeighborLoader(data, [3, 2], quant=quant.constants(8, a_z=1), **kw)                 # 0 becomes 1 / 128
    with pytest.raises(ValueError, match="quant"):
        pyg_lite.NeighborLoader(data, [3, 2], quant=replace(quant.constants(8), w_qbits=3), **kw)
    for a_s in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="quant"):
            pyg_lite.NeighborLoader(data, [3, 2], quant=quant.constants(8, a_s=a_s), **kw)
    with pytest.raises(ValueError, match="quant"):
        pyg_lite.NeighborLoader(data, [3, 2], quant=object(), **kw)                                   # carries no constants
    with pytest.raises(ValueError, match="float32"):
        pyg_lite.NeighborLoader(data, [3, 2], quant=quant.constants(8), dtype=torch.float16, **kw)   # the fp32 requirement stays
    # the published constants pass the validation: the constructor goes on to where pad=True without quant= gets on host
    # data -- the loader's CSR, the first thing that needs a device
    for bits in (8, 4, 2, 1):
        pyg_lite.check_pad_quant(quant.constants(bits))
        with pytest.raises(ValueError, match="on the GPU") as with_q:
            pyg_lite.NeighborLoader(data, [3, 2], quant=quant.constants(bits), **kw)
        with pytest.raises(ValueError, match="on the GPU") as without:
            pyg_lite.NeighborLoader(data, [3, 2], **kw)
        assert str(with_q.value) == str(without.value) and "quant" not in str(with_q.value)
