"""Node batches ready for the quantised layers, without a GPU: the header declares sgx_node_batch_quant and
sgx_node_batch_sample_quant next to the rule they follow, the ctypes mirror has the layout of the struct compiled as C,
the argument errors of the quantiser's arguments come back before anything reaches a device, the loader refuses `quant`
where it cannot hold, and the torch restatement the GPU tests compare with shows the two cases they must contain."""
import ctypes
import os
import re
import subprocess
from dataclasses import replace

import pytest
import torch

import _node_batch_quant_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgx.h")


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_header_declares_the_struct_and_the_function_behind_sgx_node_batch(L):
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+SGX_VERSION\s+(\d+)", text).group(1)) == 110 == L.lib.sgx_version()
    at = text.index("} sgx_node_batch;")
    assert "sgx_node_batch_quant" not in text[:at]                  # sgx_node_batch and everything above it: untouched
    tail = text[at:]
    struct = tail[tail.index("typedef struct sgx_node_batch_quant {"):tail.index("} sgx_node_batch_quant;")]
    for field in ("int32_t n_sets;", "int32_t qbits;", "inv_scale_adj[2], zero_adj[2];", "*values_q[2];", "*dead_row_q[2];",
                  "*values_lean[2];", "int32_t has_dead_rows_q[2];"):
        assert field in struct, field
    assert "int sgx_node_batch_sample_quant(sgx_node_batch *b, sgx_node_batch_quant *q, void *stream);" in tail
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    assert "sgx_node_batch_sample_quant" in L.SYMBOLS and " T sgx_node_batch_sample_quant\n" in out


def test_ctypes_mirror_has_the_layout_of_the_struct_compiled_as_c(L, tmp_path):
    fields = [n for n, _ in L.NodeBatchQuant._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
                   ' printf("sizeof %zu\\n", sizeof(sgx_node_batch_quant));\n'
                   + "".join(f' printf("{n} %zu\\n", offsetof(sgx_node_batch_quant, {n}));\n' for n in fields)
                   + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            name, v = ln.split()
            seen += 1
            if name == "sizeof":
                assert ctypes.sizeof(L.NodeBatchQuant) == int(v)
            else:
                assert getattr(L.NodeBatchQuant, name).offset == int(v), name
    assert seen == 1 + len(fields)
    assert fields == ["n_sets", "qbits", "inv_scale_adj", "zero_adj", "values_q", "dead_row_q", "values_lean", "has_dead_rows_q"]


def test_argument_errors_come_back_before_a_device_is_touched(L):
    call = L.lib.sgx_node_batch_sample_quant
    b, q = L.NodeBatch(), L.NodeBatchQuant()
    assert call(None, ctypes.byref(q), None) == -1 and call(ctypes.byref(b), None, None) == -1     # SGX_ERR_NULL
    q.n_sets, q.qbits = 2, 8
    q.values_q[0] = q.values_q[1] = q.dead_row_q[0] = q.dead_row_q[1] = 256
    b.dtype = 0
    assert call(ctypes.byref(b), ctypes.byref(q), None) == -3       # SGX_F16: SGX_ERR_UNSUPPORTED
    b.dtype = 1
    for n_sets in (0, 3, -1):
        q.n_sets = n_sets
        assert call(ctypes.byref(b), ctypes.byref(q), None) == -2, n_sets          # SGX_ERR_SHAPE
    q.n_sets = 2
    for qbits in (0, 3, 5, 16, 32, -8):
        q.qbits = qbits
        assert call(ctypes.byref(b), ctypes.byref(q), None) == -2, qbits
    for qbits in (8, 4, 2, 1):
        q.qbits = qbits
        for name in ("values_q", "dead_row_q"):
            for k in (0, 1):
                getattr(q, name)[k] = None
                assert call(ctypes.byref(b), ctypes.byref(q), None) == -1, (name, k)
                getattr(q, name)[k] = 256
        q.n_sets = 1                                                # the second set is not looked at
        q.values_q[1] = q.dead_row_q[1] = None
        # past the quantiser's arguments the batch's own checks answer, as in sgx_node_batch_sample: no fan-outs
        assert call(ctypes.byref(b), ctypes.byref(q), None) == L.lib.sgx_node_batch_sample(ctypes.byref(b), None) == -1
        q.n_sets = 2
        q.values_q[1] = q.dead_row_q[1] = 256
    # values_lean is optional: with everything else of q in place the answer is again the batch's
    assert q.values_lean[0] is None and call(ctypes.byref(b), ctypes.byref(q), None) == -1
    fan, hn, he = (ctypes.c_int32 * 2)(10, 10), (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    b.fanouts, b.hop_nodes, b.hop_edges = fan, hn, he
    b.n_nodes, b.nnz, b.batch, b.n_hops = 3000, 50000, 128, 2
    assert call(ctypes.byref(b), ctypes.byref(q), None) == -2       # capacities below the bounds (sgx_node_batch_sample's)
    assert list(q.has_dead_rows_q) == [0, 0]


def test_loader_refuses_quant_without_prepare_or_in_fp16():
    """The checks stand before anything is built, so tensors on the CPU reach them."""
    from sgracex1_amd import pyg_lite, quant
    qc = quant.constants(8)
    data = pyg_lite.NodeData(torch.zeros(4, 3), torch.zeros((2, 0), dtype=torch.int64))
    with pytest.raises(ValueError, match="prepare"):
        pyg_lite.NeighborLoader.__init__(pyg_lite.NeighborLoader.__new__(pyg_lite.NeighborLoader), data, [2], quant=qc)
    with pytest.raises(ValueError, match="float32"):
        pyg_lite.NeighborLoader.__init__(pyg_lite.NeighborLoader.__new__(pyg_lite.NeighborLoader), data, [2],
                                         prepare="sym_norm2", dtype=torch.float16, quant=qc)


def test_the_two_layers_of_the_demo_share_one_adjacency_constant_set():
    """ops.sample_node_batch passes one set where the keys of qc and qc.second_layer() are equal; an override that makes
    them differ gives two."""
    from sgracex1_amd import ops, quant
    for bits in (8, 4, 2, 1):
        qc = quant.constants(bits)
        assert ops._adj_quant_key(qc) == ops._adj_quant_key(qc.second_layer()) == (bits, qc.a_s, qc.a_z)
    assert ops._adj_quant_key(replace(qc, a_s=0.5)) != ops._adj_quant_key(qc)


@pytest.mark.parametrize("name", ["seeded", "hub"])
def test_restatement_on_the_gpu_tests_batches_is_not_empty(name):
    """What tests/test_gpu_node_batch_quant.py relies on, shown by the restatement alone (numpy sampler and sym_norm2
    rule, torch quantiser) for the graphs, seeds and fan-outs it uses: fill = 0 leaves dead rows, and with one bit some
    live row loses an entry to rounding (fill = 1) wherever _node_batch_quant_ref.LOSES says one can."""
    from sgracex1_amd import quant, sgrace
    rowptr, col = Q.GRAPHS[name]()
    assert len(Q.SEEDS[name]) == Q.BATCH == len(set(Q.SEEDS[name]))
    for f, fanouts in enumerate(Q.FANOUTS):
        for fill in (0, 1):
            q_ptr, q_col, val = Q.restated_batch(rowptr, col, Q.SEEDS[name], fanouts, fill, Q.weights_of(name, len(col)))
            n, val = len(q_ptr) - 1, torch.as_tensor(val)
            row = Q.rows_of(q_ptr)
            for bits in (8, 4, 2, 1):
                qc = quant.constants(bits)
                vq = sgrace._fq_unsigned(val, qc.a_s, qc.a_z, bits)
                dead = Q.dead_rows(vq, row, n)
                lost = int(((vq == 0) & (val > 0) & ~dead[row]).sum())
                if fill == 0:
                    assert 0 < int(dead.sum()) < n, (fanouts, bits)           # the last hop's rows: a loop of weight 0
                elif bits == 1:
                    assert (lost > 0) == Q.LOSES[name, f], (fanouts, lost)
