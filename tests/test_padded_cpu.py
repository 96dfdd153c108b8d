"""Padded batches without a GPU: the capacity rule against brute force over every B-subset of the 7-graph set, the
filler layout of tests/_padded_ref.py against the rule's formulas, the padding loader's batches against the plain
loader's, and the argument errors of sgx_collate_graphs_padded and sgx_batch_plan_regroup."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import _padded_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, NULL, UNSUPPORTED = -2, -1, -3


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


class _Set:
    """What ops.pad_capacity and the loader's host side read of an ops.GraphSet."""

    def __init__(self, cs):
        self.counts = cs[:4]
        self._sym_norm2 = type("Prepared", (), {"counts": cs[4]})()

    def __len__(self):
        return len(self.counts[0])


def test_new_symbols_and_the_pad_struct(L, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_collate_graphs_padded", "sgx_batch_plan_regroup"):
        assert name in L.SYMBOLS and f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
                   ' printf("size %zu\\n", sizeof(sgx_collate_pad));\n'
                   + "".join(f' printf("{n} %zu\\n", offsetof(sgx_collate_pad, {n}));\n' for n, _ in L.CollatePad._fields_)
                   + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).split("\n") if ln)
    assert int(lines.pop("size")) == ctypes.sizeof(L.CollatePad)
    assert {n: int(v) for n, v in lines.items()} == {n: getattr(L.CollatePad, n).offset for n, _ in L.CollatePad._fields_}


@pytest.mark.parametrize("B", [3, 4])
def test_capacity_rule_against_every_subset(L, B):
    from sgracex1_amd import ops
    cs = R.counts()
    cap = ops.pad_capacity(_Set(cs), B)
    assert {k: v for k, v in cap.__dict__.items()} == R.capacity(cs, B)
    rows, edges, adj, fea, norm = cs
    F = cap.n_graphs - B
    seen = {k: 0 for k in ("n", "P", "E", "f")}
    for sub in itertools.combinations(range(R.N_SET), B):
        sub = list(sub)
        n = int(rows[sub].sum())
        P = cap.n_rows - n
        assert cap.fits(B, n) and 0 <= P <= F * cap.filler_rows
        assert edges[sub].sum() <= cap.n_edges and fea[sub].sum() <= cap.nnz_fea
        assert adj[sub].sum() + P <= cap.nnz_adj and norm[sub].sum() + P <= cap.nnz_norm
        seen = {"n": max(seen["n"], n), "P": max(seen["P"], P), "E": max(seen["E"], int(edges[sub].sum())),
                "f": max(seen["f"], int(fea[sub].sum()))}
    # nothing to spare where the rule says "the sum of the B largest": some subset reaches each capacity
    assert seen == {"n": cap.n_rows, "P": cap.n_rows - cap.n_min, "E": cap.n_edges, "f": cap.nnz_fea}
    assert (F - 1) * cap.filler_rows < seen["P"] or F == 0
    assert not cap.fits(B - 1, 1) and not cap.fits(B, cap.n_rows + 1)


def test_capacity_with_pad_rows_and_its_errors(L):
    from sgracex1_amd import ops
    cs = R.counts()
    s = _Set(cs)
    full = ops.pad_capacity(s, 3)
    cap = ops.pad_capacity(s, 3, pad_rows=full.n_rows - 4)
    assert cap.__dict__ == R.capacity(cs, 3, full.n_rows - 4)
    assert cap.n_rows == full.n_rows - 4 and cap.nnz_adj == full.nnz_adj - 4 and cap.n_edges == full.n_edges
    fit = [sub for sub in itertools.combinations(range(R.N_SET), 3) if cap.fits(3, int(cs[0][list(sub)].sum()))]
    assert 0 < len(fit) < 35                       # some batches are over pad_rows and arrive unpadded
    for sub in fit:
        assert cap.n_rows - cs[0][list(sub)].sum() <= (cap.n_graphs - 3) * cap.filler_rows
    with pytest.raises(ValueError):
        ops.pad_capacity(s, 3, pad_rows=full.n_min - 1)
    for B in (0, R.N_SET + 1):
        with pytest.raises(ValueError):
            ops.pad_capacity(s, B)


def _live(n, a, f, E, B, rng):
    """An unpadded batch of the right shapes with arbitrary contents (the layout does not look at them)."""
    cut = np.sort(rng.integers(0, n + 1, B - 1))
    return dict(x=rng.random((n, 7), np.float32), edge_index=rng.integers(0, n, (2, E)), batch=np.zeros(n, np.int64),
                y=np.ones(B, np.int64), graph_ptr=np.concatenate([[0], cut, [n]]).astype(np.int32),
                adj_rowptr=np.linspace(0, a, n + 1).astype(np.int32), adj_col=rng.integers(0, n, a).astype(np.int32),
                adj_val={"f32": rng.random(a, np.float32) + 1, "f16": (rng.random(a) + 1).astype(np.float16)},
                fea_rowptr=np.linspace(0, f, n + 1).astype(np.int32), fea_col=rng.integers(0, 7, f).astype(np.int32),
                fea_val={"f32": rng.random(f, np.float32) + 1})


@pytest.mark.parametrize("n", [20, 14, 11, 6])      # P = 0; a partly filled last filler; a full one and an empty; the largest P
def test_filler_layout_restated(n):
    """Validates the REFERENCE itself: tests/_padded_ref.padded against the rule's formulas, written a second way.  It
    calls nothing from the package (it passes without the feature) and is no coverage of the kernel, which
    tests/test_gpu_padded.py holds to this reference element for element."""
    cap = R.capacity(R.counts(), 3)
    N, G, Rf, B = cap["n_rows"], cap["n_graphs"], cap["filler_rows"], 3
    a, f, E = 17, n, 30
    out = R.padded(_live(n, a, f, E, B, np.random.default_rng(n)), cap, 7)
    P = N - n
    gp = out["graph_ptr"]
    assert len(gp) == G + 1 and gp[B] == n and gp[G] == N and (np.diff(gp) >= 0).all()
    sizes = np.diff(gp)[B:]
    assert list(sizes) == [min(max(P - k * Rf, 0), Rf) for k in range(G - B)]
    assert (out["batch"][n:] == np.repeat(np.arange(B, G), sizes)).all()           # batch and graph_ptr say the same
    assert not out["x"][n:].any() and (out["y"][B:] == 0).all() and len(out["y"]) == G
    rp, col = out["adj_rowptr"], out["adj_col"]
    assert len(rp) == N + 1 and rp[N] == a + P and len(col) == cap["nnz_adj"]
    for j in range(P):
        assert rp[n + j] == a + j and rp[n + j + 1] - rp[n + j] == 1 and col[a + j] == n + j
    for v in out["adj_val"].values():
        assert (v[a:a + P] == 1).all() and not v[a + P:].any()
    assert not col[a + P:].any()
    assert (out["fea_rowptr"][n:] == f).all() and len(out["fea_rowptr"]) == N + 1 and not out["fea_col"][f:].any()
    assert (out["edge_index"][:, E:] == -1).all() and out["edge_index"].shape == (2, cap["n_edges"])


def _loader(pad, pad_rows=None, B=3, seed=5):
    """A GraphLoader's host side over the 7-graph set's counts (the device side needs a GPU: tests/test_gpu_padded.py)."""
    from sgracex1_amd import ops, pyg_lite as G
    ld = G.GraphLoader.__new__(G.GraphLoader)
    ld.graphs, ld.batch_size, ld.shuffle = _Set(R.counts()), B, True
    ld.generator = torch.Generator().manual_seed(seed)
    ld.pad, ld.extras = pad, None
    ld.capacity = ops.pad_capacity(ld.graphs, B, pad_rows) if pad else None
    return ld


def test_padding_loader_draws_the_plain_loaders_batches():
    plain, pad, tight = _loader(False), _loader(True), _loader(True, pad_rows=12)
    rows = R.counts()[0]
    some_over = False
    for _ in range(3):                              # three epochs from the same generator state
        want = plain.batches()
        assert [len(b) for b in want] == [3, 3, 1]
        for ld in (pad, tight):
            got = ld.batches()
            assert all((g == w).all() for g, w in zip(got, want)) and len(got) == len(want)
            for ids in got:
                fits = len(ids) == 3 and rows[ids].sum() <= ld.capacity.n_rows
                assert ld.padded(ids) == fits
                some_over |= len(ids) == 3 and not fits
        assert not any(plain.padded(ids) for ids in want)
        assert [pad.padded(ids) for ids in want] == [True, True, False]      # the short last batch arrives unpadded
    assert some_over                                # pad_rows = 12: a full batch over it arrives unpadded


def test_a_prepared_padding_loader_hands_dead_row_batches_over_unpadded():
    ld = _loader(True)
    dead = np.zeros(R.N_SET, bool)
    dead[[0, 6]] = True
    ld.extras = type("Extras", (), {"prepared": type("Prepared", (), {"has_dead": dead})()})()
    assert ld.padded([1, 2, 5]) and not ld.padded([0, 2, 3]) and not ld.padded([1, 6, 2]) and not ld.padded([1, 2])


def test_loader_refuses_pad_with_quant_before_touching_the_device():
    from sgracex1_amd import pyg_lite as G
    with pytest.raises(ValueError, match="quant"):
        G.GraphLoader([], batch_size=3, prepare="sym_norm2", dtypes=(torch.float32,), quant=object(), pad=True)
    with pytest.raises(ValueError, match="pad_rows"):
        G.GraphLoader([], batch_size=3, pad_rows=10)


def _args(L, n_extras=0):
    s = L.GraphSet()
    s.n_graphs, s.n_feat, s.n_edges = 7, 7, 10
    for name, _ in L.GraphSet._fields_[3:]:
        setattr(s, name, 256)
    b = L.GraphBatch()
    b.n_graphs = 3
    for name, _ in L.GraphBatch._fields_[5:]:
        if not name.startswith("values"):
            setattr(b, name, 256)
    xs = (L.CollateExtra * L.SGX_COLLATE_MAX_EXTRAS)()
    for k in range(n_extras):
        for name in ("rowPtr", "columnIndex", "values", "entry_off", "rowPtr_out", "columnIndex_out"):
            setattr(xs[k], name, 256)
    p = L.CollatePad()
    p.n_rows, p.n_graphs, p.filler_rows, p.n_edges, p.nnz_adj, p.nnz_fea = 20, 5, 9, 74, 40, 20
    for k in range(L.SGX_COLLATE_MAX_EXTRAS):
        p.nnz_extra[k] = 60
    return s, b, xs, p


def test_padded_collation_argument_errors_need_no_gpu(L):
    def run(s, b, xs, p, n=0):
        ref = lambda v: None if v is None else ctypes.byref(v)
        return L.lib.sgx_collate_graphs_padded(ref(s), ref(b), xs, n, ref(p), None)

    s, b, xs, p = _args(L)
    assert run(s, b, xs, None) == NULL and run(None, b, xs, p) == NULL and run(s, None, xs, p) == NULL
    assert run(s, b, xs, p, -1) == SHAPE and run(s, b, xs, p, L.SGX_COLLATE_MAX_EXTRAS + 1) == SHAPE
    assert run(s, b, None, p, 1) == NULL
    # the collator's own errors, with the capacities where its totals stand
    for field in ("n_rows", "n_edges", "nnz_adj", "nnz_fea"):
        s, b, xs, p = _args(L)
        setattr(p, field, -1)
        assert run(s, b, xs, p) == SHAPE, field
    for field in ("index", "node_off", "x", "edge_index", "batch", "y", "graph_ptr", "rowPtr_adj", "columnIndex_adj", "rowPtr_fea"):
        s, b, xs, p = _args(L)
        setattr(b, field, None)
        assert run(s, b, xs, p) == NULL, field
    s, b, xs, p = _args(L)
    b.n_rows, b.n_edges, b.nnz_adj, b.nnz_fea = -1, -1, -1, -1          # the batch's own totals are not read
    s.n_graphs = 0
    assert run(s, b, xs, p) == SHAPE
    # capacities smaller than the filler rule needs
    for field, value in (("n_graphs", 2),            # G < B
                         ("filler_rows", -1),
                         ("filler_rows", 3),         # G R_f = 15 < N = 20: the fillers cannot hold what is left
                         ("nnz_adj", 2 ** 31)):
        s, b, xs, p = _args(L)
        setattr(p, field, value)
        assert run(s, b, xs, p) == SHAPE, (field, value)
    s, b, xs, p = _args(L)
    p.n_rows, p.n_graphs, p.filler_rows = 40, 10, 4         # every batch leaves 40 - 3 * 4 = 28 rows to the fillers
    p.nnz_adj = 27
    assert run(s, b, xs, p) == SHAPE
    s, b, xs, p = _args(L, 1)
    p.n_rows, p.n_graphs, p.filler_rows, p.nnz_adj = 40, 10, 4, 28
    p.nnz_extra[0] = 27
    assert run(s, b, xs, p, 1) == SHAPE
    # extras: the existing checks, and a values-only extra is refused
    s, b, xs, p = _args(L, 1)
    xs[0].entry_off = None
    assert run(s, b, xs, p, 1) == NULL
    s, b, xs, p = _args(L, 2)
    xs[1].rowPtr_out = xs[1].columnIndex_out = None
    assert run(s, b, xs, p, 2) == UNSUPPORTED


def test_regroup_argument_errors_need_no_gpu(L):
    lib = L.lib
    assert lib.sgx_batch_plan_regroup(None, None, None) == NULL
    h = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create_ex(0, 0, 0, None, None, None, 16, L.SGX_BATCH_BACKWARD, ctypes.byref(h), None) == 0
    try:
        assert lib.sgx_batch_plan_regroup(h, None, None) == UNSUPPORTED          # the plan owns its table
    finally:
        lib.sgx_batch_plan_destroy(h)
    k = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create_known(0, 0, 0, None, 0, 16, L.SGX_BATCH_BACKWARD, None, ctypes.byref(k), None) == 0
    try:
        assert lib.sgx_batch_plan_regroup(k, None, None) == 0                    # a trusted plan without a table is left alone
    finally:
        lib.sgx_batch_plan_destroy(k)
