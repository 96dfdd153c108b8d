"""sgx_quant_stack_forward without a GPU: symbols, struct layout compiled as C, the argument errors that need no device,
and the float32 chain reference of the GPU tests (tests/_quant_stack_ref.py) pinned, stage by stage, to the dense
emulation in sgracex1_amd/sgrace.py (config.acc = 0, fake_quantization = 1) -- this project's restatement of the reference,
and not the code under test.  Parity of the quantised layer itself is unpinned: the reference records no quantised output."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _gat_ref as R
import _quant_ref as Q
import _quant_stack_ref as QS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ["sgx_quant_stack_workspace_bytes", "sgx_quant_stack_forward"]


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_new_symbols_are_exported(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in NEW:
        assert name in L.SYMBOLS
        assert f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110


def test_quant_stack_structs_match_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof_layer %zu\\n", sizeof(sgx_quant_stack_layer));\n'
        ' printf("sizeof_desc %zu\\n", sizeof(sgx_quant_stack_desc));\n'
        + "".join(f' printf("l.{n} %zu\\n", offsetof(sgx_quant_stack_layer, {n}));\n' for n, _ in L.QuantStackLayer._fields_)
        + "".join(f' printf("d.{n} %zu\\n", offsetof(sgx_quant_stack_desc, {n}));\n' for n, _ in L.QuantStackDesc._fields_)
        + " return SGX_VERSION == 110 ? 0 : 1;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        seen += 1
        if name == "sizeof_layer":
            assert ctypes.sizeof(L.QuantStackLayer) == int(val)
        elif name == "sizeof_desc":
            assert ctypes.sizeof(L.QuantStackDesc) == int(val)
        elif name.startswith("l."):
            assert getattr(L.QuantStackLayer, name[2:]).offset == int(val), name
        else:
            assert getattr(L.QuantStackDesc, name[2:]).offset == int(val), name
    assert seen == 2 + len(L.QuantStackLayer._fields_) + len(L.QuantStackDesc._fields_)
    # sgx_gat_stack_layer field for field, then the quantiser; the descriptor up to the layer array as sgx_gat_stack_desc
    names = [n for n, _ in L.QuantStackLayer._fields_]
    assert names == [n for n, _ in L.GatStackLayer._fields_] + ["quant"]
    for n, _ in L.GatStackLayer._fields_:
        assert getattr(L.QuantStackLayer, n).offset == getattr(L.GatStackLayer, n).offset, n
    for n, _ in L.GatStackDesc._fields_[:[f for f, _ in L.GatStackDesc._fields_].index("layer") + 1]:
        assert getattr(L.QuantStackDesc, n).offset == getattr(L.GatStackDesc, n).offset, n


def _desc(L, n_layers=2, dtype=1):
    d = L.QuantStackDesc()
    d.dtype, d.n_layers = dtype, n_layers
    for l in range(4):
        d.layer[l].gemm_mode, d.layer[l].M_fea, d.layer[l].P_w = 1, 8, 8
    return d


def _quant(L, bits=8):
    from sgracex1_amd import quant
    return quant.constants(bits).as_struct(nnz_adj=0)


def test_argument_errors_need_no_gpu(L):
    """Every pointer is NULL or a made-up address, the plan is the empty batch's: nothing may be launched."""
    lib = L.lib
    fwd = lambda d: lib.sgx_quant_stack_forward(ctypes.byref(d), None)
    size = lambda d: lib.sgx_quant_stack_workspace_bytes(ctypes.byref(d))
    assert lib.sgx_quant_stack_forward(None, None) == -1                    # SGX_ERR_NULL
    assert lib.sgx_quant_stack_workspace_bytes(None) == 0
    for n in (0, 5):
        assert fwd(_desc(L, n)) == -2                                        # SGX_ERR_SHAPE
    assert fwd(_desc(L)) == -1                                               # no plan
    assert fwd(_desc(L, dtype=7)) == -3
    h = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create(1, 0, 0, None, None, None, 64, ctypes.byref(h), None) == 0 and h.value
    try:
        d = _desc(L)
        d.plan = h
        assert fwd(d) == -1                                                  # B missing
        for l in range(2):
            d.layer[l].B = 256
        assert fwd(d) == 0 and size(d) == 0                                  # every quant NULL: sgx_gat_stack_forward
        d.layer[1].gat_mode = 1
        assert fwd(d) == -1                                                  # its errors: attention NULL on a GAT layer
        d.layer[1].attention = 512
        q = _quant(L)
        d.layer[1].quant = ctypes.pointer(q)
        assert fwd(d) == 0 and size(d) == 0                                  # the empty batch: nothing runs
        d.dtype = 0
        assert fwd(d) == -3 and size(d) == 0                                 # a quantiser on fp16 layers
        d.dtype = 1
        for bits in (0, 3, 5, 7, 9, 16):
            q.qbits = bits
            assert fwd(d) == -3, bits                                        # qbits outside {8, 4, 2, 1}
        for bits in (8, 4, 2, 1):
            q.qbits = bits
            assert fwd(d) == 0, bits
        q.flags = L.SGX_QUANT_INT8 | L.SGX_QUANT_INT8_AUTO                    # ignored: the stack takes the fp32 form
        assert fwd(d) == 0
        q.zero_adj = 1.0
        assert fwd(d) == -3
        q.zero_adj, q.zero_fea = 0.0, 1.0
        assert fwd(d) == 0                                                   # a dense layer may have a zero point ...
        q0 = _quant(L)
        q0.zero_fea = 1.0
        d.layer[0].quant, d.layer[0].gemm_mode = ctypes.pointer(q0), 0
        assert fwd(d) == -3                                                  # ... a sparse layer 0 may not
        q0.zero_fea = 0.0
        assert fwd(d) == 0
        q0.scale_fea = 31
        assert fwd(d) == -3
        q0.scale_fea, q0.internal_bits = 4, 0
        assert fwd(d) == -3
        q0.internal_bits = 16
        d.layer[2].quant = ctypes.pointer(_quant(L, 8))
        d.layer[2].quant.contents.qbits = 3                                  # past n_layers: not looked at
        assert fwd(d) == 0
    finally:
        assert lib.sgx_batch_plan_destroy(h) == 0


# ---- the reference of the GPU tests against the dense emulation ---------------------------------------------------------
def _mutag_batch(n=12):
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs[:n])


@pytest.mark.parametrize("gat", [0, 1])
@pytest.mark.parametrize("bits", [8, 4])
def test_chain_reference_against_the_dense_emulation(bits, gat):
    """GAT_POOL_PYNQ under config.acc = 0, fake_quantization = 1 on a 12-graph MUTAG batch, stage by stage: each layer of
    the emulation lies inside the reference's bound on the emulation's own input (H is exact, so the bound is stage 2's:
    an fp32 sum in any order), the readout inside readout_f64's.  The emulation quantises both layers with the first
    layer's constants; at 8 and 4 bits second_layer() holds the same numbers (quant._RANGES), which is asserted."""
    from sgracex1_amd import config, quant, sgrace
    saved = config.snapshot()
    try:
        config.acc, config.fake_quantization, config.w_qbits, config.compute_attention = 0, 1, bits, gat
        config.float_type = np.float32
        sgrace.init_SGRACE()
        qc = sgrace.quant_constants
        assert qc == quant.constants(bits)
        q2 = qc.second_layer()
        assert (q2.w_s, q2.w_z, q2.f_s, q2.f_z, q2.scale_fea, q2.deq_o) == (qc.w_s, qc.w_z, qc.f_s, qc.f_z, qc.scale_fea, qc.deq_o)
        torch.manual_seed(3)
        model = sgrace.GAT_POOL_PYNQ(7, 20, 2).eval()
        b = _mutag_batch()
        with torch.no_grad():
            ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
            adj = torch.sparse_coo_tensor(ei, norm, (b.num_nodes, b.num_nodes))
            d1 = model.reluh(model.att1(gat, 0, 1, b.x, ei, norm, adj))
            d2 = model.att2(gat, 1, 0, d1, ei, norm, adj)
            logits = model(b.x, b.edge_index, b.batch)
        # the same operands as CSR (sym_norm2 sorts by row, then column)
        n = b.num_nodes
        rowptr = np.zeros(n + 1, np.int64)
        np.add.at(rowptr, ei[0].numpy() + 1, 1)
        rowptr = np.cumsum(rowptr)
        col, a_val = ei[1].numpy().astype(np.int64), norm.numpy().astype(np.float32)
        ptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy(), minlength=b.num_graphs))])
        W = [model.att1.weight.detach().numpy(), model.att2.weight.detach().numpy()]
        atts = [m.attention.detach().numpy().reshape(-1) if gat else None for m in (model.att1, model.att2)]
        rows = np.arange(n)
        X = b.x.numpy()
        for l, (got, relu, c) in enumerate(((d1, True, qc), (d2, False, q2))):
            r = QS.layer_ref((rowptr, col), a_val, X, W[l], atts[l], c, relu, alpha=model.att1.alpha)
            assert r["magnitude"] < Q.EXACT_BELOW
            if gat:
                assert not r["dead"].any()                                # (the emulation gives a dead row the mean, not 0)
            assert np.isfinite(r["bound"]).all()
            Q.check_D(got.numpy(), r["D"], r["bound"])
            X = got.numpy()
        assert (np.abs(d2.numpy()) > 0).mean() > 0.5                          # the layers computed something
        hw, hb = model.lin.weight.detach().numpy(), model.lin.bias.detach().numpy()
        _p, wl, _bP, bL = QS.readout_f64(d2.numpy(), ptr, hw, hb)
        R.check("logits", logits.double().numpy(), wl, bL, np.arange(len(wl)), {})
        # chain() is those stages strung together: its first layer is layer_ref's, and its logits lie near the emulation's
        # (a D_1 element that differs in the last place may move a grid step of layer 2: no bound is claimed end to end)
        ch = QS.chain((rowptr, col), a_val, b.x.numpy(), W, atts, [True, False], ptr, [qc, q2], hw, hb, alpha=model.att1.alpha)
        first = QS.layer_ref((rowptr, col), a_val, b.x.numpy(), W[0], atts[0], qc, True, alpha=model.att1.alpha)
        assert np.array_equal(ch["outs"][0], first["D"].astype(np.float32))
        assert ch["logits"].shape == wl.shape and np.isfinite(ch["logits"]).all()
    finally:
        config.restore(saved)
        sgrace.init_SGRACE()
