"""Padded batches that carry the quantised adjacencies, without a GPU (include/sgx.h, sgx_collate_graphs_padded_quant):
the numpy restatement of tests/_padded_quant_ref.py on a hand-written batch, the call's two preconditions on the published
constants, the new symbol and struct against the C compiler, every argument error on made-up addresses, and the loader's
host checks."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest
import torch

import _padded_quant_ref as RQ
from test_padded_cpu import _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, NULL, UNSUPPORTED = -2, -1, -3


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_restatement_on_a_hand_written_batch():
    """Three graphs of 2, 1 and 3 rows at N = 9 in G = 5 graphs of up to R_f = 3 rows: P = 3 filler rows, 8 live entries of
    the normalised pattern and a capacity of 13."""
    from sgracex1_amd import quant
    c8, c2 = quant.constants(8), quant.constants(2)
    cap = dict(batch_size=3, n_rows=9, n_graphs=5, filler_rows=3, n_edges=6, nnz_adj=9, nnz_fea=7, nnz_norm=13)
    n = 6
    norm_val = np.array([0.5, 0.5, 1.0, 0.25, 0.5, 0.5, 0.25, 1.0], np.float32)
    q8, q2 = RQ.Q.quantise_adj(norm_val, c8), RQ.Q.quantise_adj(norm_val, c2)
    live = dict(x=np.ones((n, 2), np.float32), edge_index=np.array([[0, 1, 3, 4], [1, 0, 4, 3]]), batch=np.array([0, 0, 1, 2, 2, 2]),
                y=np.array([1, 0, 1]), graph_ptr=np.array([0, 2, 3, 6], np.int32),
                adj_rowptr=np.array([0, 1, 2, 2, 3, 4, 4], np.int32), adj_col=np.array([1, 0, 4, 3], np.int32),
                adj_val={"f32": np.ones(4, np.float32)},
                fea_rowptr=np.arange(n + 1, dtype=np.int32), fea_col=np.zeros(n, np.int32), fea_val={"f32": np.ones(n, np.float32)},
                norm_rowptr=np.array([0, 2, 4, 5, 6, 7, 8], np.int32), norm_col=np.array([0, 1, 0, 1, 2, 4, 3, 5], np.int32),
                norm_val={"f32": norm_val}, norm_dead=np.zeros(n, bool),
                q_val={RQ.key(c8): q8, RQ.key(c2): q2},
                q_dead={RQ.key(c8): np.zeros(n, bool), RQ.key(c2): np.array([0, 0, 0, 1, 0, 0], bool)})
    out = RQ.padded(live, cap, 2, (c8, c2))
    assert list(out["norm_rowptr"]) == [0, 2, 4, 5, 6, 7, 8, 9, 10, 11] and list(out["norm_col"][8:]) == [6, 7, 8, 0, 0]
    # 8 bits: 1 / a_s = 255, the 1 clips to the grid's top 255 / 128; 2 bits: 1 / a_s = 30, the top is 3 / 2
    assert list(out["q_val"][RQ.key(c8)][8:]) == [255 / 128] * 3 + [0.0] * 2
    assert list(out["q_val"][RQ.key(c2)][8:]) == [1.5] * 3 + [0.0] * 2
    for c, q in ((c8, q8), (c2, q2)):
        v, d = out["q_val"][RQ.key(c)], out["q_dead"][RQ.key(c)]
        assert v.dtype == np.float32 and v.shape == (13,) and np.array_equal(v[:8], q)
        assert d.dtype == bool and d.shape == (9,) and np.array_equal(d[:6], live["q_dead"][RQ.key(c)]) and not d[6:].any()
    # every other array is tests/_padded_ref.padded's
    plain = RQ.R.padded(live, cap, 2)
    assert all(np.array_equal(out[k], v) for k, v in plain.items() if not isinstance(v, dict))


@pytest.mark.parametrize("bits", [8, 4, 2, 1])
def test_published_constants_keep_the_fillers_inert(bits):
    """fq(1) > 0 and fq(0) == 0 on the adjacency grid of both layers' constants, by the restatement and by the scalar rule
    the loader checks with; 0 stays 0 on their feature grids (pyg_lite.check_pad_quant_features)."""
    from sgracex1_amd import pyg_lite as G, quant
    qc = quant.constants(bits)
    for c in (qc, qc.second_layer()):
        assert RQ.inert(c)
        one, zero = (G._fq_unsigned_scalar(v, c.a_s, c.a_z, bits) for v in (1.0, 0.0))
        assert one == float(RQ.fq(1.0, c)) > 0 and zero == float(RQ.fq(0.0, c)) == 0
        assert G._fq_unsigned_scalar(0.0, c.f_s, c.f_z, bits) == 0
    G.check_pad_quant(qc)
    G.check_pad_quant_features(qc)


def test_new_symbol_and_struct(L, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    name = "sgx_collate_graphs_padded_quant"
    assert name in L.SYMBOLS and f" T {name}\n" in out
    assert L.lib.sgx_version() == 110
    S = L.CollatePadQuant
    assert [n for n, _ in S._fields_] == ["qbits", "inv_scale_adj", "zero_adj"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
                   ' printf("size %zu\\n", sizeof(sgx_collate_pad_quant));\n'
                   + "".join(f' printf("{n} %zu\\n", offsetof(sgx_collate_pad_quant, {n}));\n' for n, _ in S._fields_)
                   + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).split("\n") if ln)
    assert int(lines.pop("size")) == ctypes.sizeof(S)
    assert {n: int(v) for n, v in lines.items()} == {n: getattr(S, n).offset for n, _ in S._fields_}
    fn = L.lib.sgx_collate_graphs_padded_quant
    assert len(fn.argtypes) == 7 and fn.argtypes[5] == ctypes.POINTER(S)


def _quant_args(L, n_extras=2, bits=8):
    """test_padded_cpu's made-up arguments with extras 1 .. n_extras - 1 values-only, on the published 8-bit grid."""
    from sgracex1_amd import quant
    s, b, xs, p = _args(L, n_extras)
    q = L.CollatePadQuant()
    c = quant.constants(bits)
    for k in range(1, n_extras):
        xs[k].rowPtr_out = xs[k].columnIndex_out = None
        xs[k].values_out[1] = 256
    for k in range(L.SGX_COLLATE_MAX_EXTRAS):
        q.qbits[k], q.inv_scale_adj[k], q.zero_adj[k] = bits, 1 / c.a_s, c.a_z
    return s, b, xs, p, q


def test_argument_errors_need_no_gpu(L):
    ref = lambda v: None if v is None else ctypes.byref(v)

    def run(s, b, xs, p, q, n):
        return L.lib.sgx_collate_graphs_padded_quant(ref(s), ref(b), xs, n, ref(p), ref(q), None)

    s, b, xs, p, q = _quant_args(L)
    assert run(s, b, xs, p, q, -1) == SHAPE and run(s, b, xs, p, q, L.SGX_COLLATE_MAX_EXTRAS + 1) == SHAPE
    assert run(s, None, xs, p, q, 2) == NULL and run(s, b, xs, None, q, 2) == NULL and run(s, b, None, p, q, 2) == NULL
    assert run(s, b, xs, p, None, 2) == NULL                                   # q NULL with a values-only extra
    assert run(None, b, xs, p, q, 2) == NULL                                   # (the collator's own, behind the quantiser's)
    # a values-only extra with no pattern-bearing extra before it
    s, b, xs, p, q = _quant_args(L)
    xs[0].rowPtr_out = xs[0].columnIndex_out = None
    assert run(s, b, xs, p, q, 2) == SHAPE and run(s, b, xs, p, q, 1) == SHAPE
    # a capacity other than its pattern's
    s, b, xs, p, q = _quant_args(L, 3)
    p.nnz_extra[2] = p.nnz_extra[0] + 1
    assert run(s, b, xs, p, q, 3) == SHAPE
    p.nnz_extra[2] = p.nnz_extra[0] - 1
    assert run(s, b, xs, p, q, 3) == SHAPE
    # the pattern a values-only extra shares is the nearest pattern-bearing extra before it
    s, b, xs, p, q = _quant_args(L, 3)
    for name in ("rowPtr_out", "columnIndex_out"):
        setattr(xs[1], name, 256)
    p.nnz_extra[0], p.nnz_extra[1], p.nnz_extra[2] = 50, 60, 50
    assert run(s, b, xs, p, q, 3) == SHAPE
    for bits in (0, 3, 16, -8):
        s, b, xs, p, q = _quant_args(L)
        q.qbits[1] = bits
        assert run(s, b, xs, p, q, 2) == UNSUPPORTED, bits
    # the two preconditions: a 1 that rounds to 0 (a_s = 4), a 0 that does not stay 0 (zero point 1), not a number
    for inv, zero in ((0.25, 0.0), (255.0, 1.0), (float("nan"), 0.0), (255.0, float("nan"))):
        s, b, xs, p, q = _quant_args(L)
        q.inv_scale_adj[1], q.zero_adj[1] = inv, zero
        assert run(s, b, xs, p, q, 2) == UNSUPPORTED, (inv, zero)
    # constants of an extra with a pattern of its own are not read
    s, b, xs, p, q = _quant_args(L)
    q.qbits[0], q.inv_scale_adj[0] = 77, float("nan")
    s.n_graphs = 0
    assert run(s, b, xs, p, q, 2) == SHAPE                                     # (past the quantiser's checks: the set's error)
    # then everything sgx_collate_graphs_padded returns
    s, b, xs, p, q = _quant_args(L)
    xs[1].entry_off = None
    assert run(s, b, xs, p, q, 2) == NULL
    s, b, xs, p, q = _quant_args(L)
    xs[1].columnIndex_out = 256                                                 # columnIndex_out without rowPtr_out
    assert run(s, b, xs, p, q, 2) == NULL
    for field, value in (("n_graphs", 2), ("filler_rows", -1), ("filler_rows", 3), ("nnz_adj", 2 ** 31), ("n_rows", -1)):
        s, b, xs, p, q = _quant_args(L)
        setattr(p, field, value)
        assert run(s, b, xs, p, q, 2) == SHAPE, (field, value)
    s, b, xs, p, q = _quant_args(L)
    p.n_rows, p.n_graphs, p.filler_rows, p.nnz_adj = 40, 10, 4, 28             # every batch leaves 28 rows to the fillers
    p.nnz_extra[0] = p.nnz_extra[1] = 27
    assert run(s, b, xs, p, q, 2) == SHAPE
    # without a values-only extra q may be NULL, and the errors are the plain call's
    s, b, xs, p = _args(L, 1)
    s.n_graphs = 0
    assert run(s, b, xs, p, None, 1) == SHAPE and run(s, b, xs, p, None, 0) == SHAPE


def test_the_plain_padded_call_still_refuses_a_values_only_extra(L):
    s, b, xs, p, q = _quant_args(L)
    assert L.lib.sgx_collate_graphs_padded(ctypes.byref(s), ctypes.byref(b), xs, 2, ctypes.byref(p), None) == UNSUPPORTED


def test_loader_host_checks_come_before_any_device_work():
    from sgracex1_amd import pyg_lite as G, quant
    qc = quant.constants(8)
    kw = dict(batch_size=3, prepare="sym_norm2", dtypes=(torch.float32,))
    # (an empty dataset: a loader that got past its host checks would fail on it with another message)
    for bad in (dict(pad_quant=True), dict(pad_quant=True, pad=True), dict(pad_quant=True, quant=qc)):
        with pytest.raises(ValueError, match="pad_quant=True needs pad=True and quant="):
            G.GraphLoader([], **kw, **bad)
    with pytest.raises(ValueError, match=r"quant.*pad_quant=True"):
        G.GraphLoader([], **kw, quant=qc, pad=True)
    dead_one = dataclasses.replace(qc, a_s=4.0)                  # 1 / a_s = 0.25 rounds to 0: the filler rows would be dead
    weighty = dataclasses.replace(qc, a_z=1)                     # 0 becomes 1 / 128: the spare entries would carry weight
    second = dataclasses.replace(qc, f_z2=3)                     # layer 2 would read a filler row's 0 as 3 / 128
    for bad, why in ((dead_one, "rounds to 0"), (weighty, "carry weight"), (second, "would not stay inert")):
        with pytest.raises(ValueError, match="quant") as e:
            G.GraphLoader([], **kw, quant=bad, pad=True, pad_quant=True)
        assert why in str(e.value), (why, str(e.value))
    with pytest.raises(ValueError, match="quant"):
        G.GraphLoader([], **kw, quant=object(), pad=True, pad_quant=True)


def test_quantised_dead_graphs_arrive_unpadded():
    """loader.padded() on the host: a graph dead under either layer's quantised mask keeps its batch unpadded."""
    from sgracex1_amd import ops, pyg_lite as G
    from test_padded_cpu import _Set, R
    ld = G.GraphLoader.__new__(G.GraphLoader)
    ld.graphs, ld.batch_size, ld.shuffle, ld.pad, ld.pad_quant = _Set(R.counts()), 3, False, True, True
    ld.capacity = ops.pad_capacity(ld.graphs, 3)
    none, one, other = np.zeros(R.N_SET, bool), np.zeros(R.N_SET, bool), np.zeros(R.N_SET, bool)
    one[4], other[6] = True, True
    prepared = type("Prepared", (), {"has_dead": none, "quant": {"k1": (None, None, one), "k2": (None, None, other)}})()
    ld.extras = type("Extras", (), {"prepared": prepared, "keys": ("k1", "k2")})()
    assert ld.padded([1, 2, 5]) and not ld.padded([1, 4, 5]) and not ld.padded([6, 2, 5])
    ld.pad_quant = False
    assert ld.padded([1, 4, 5]) and ld.padded([6, 2, 5])
