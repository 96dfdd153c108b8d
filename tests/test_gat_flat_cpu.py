"""The entry-split GAT aggregate without a GPU: the two symbols and their derived binding, every argument error of
sgx_gat_aggregate_flat on made-up addresses (nothing is launched before the checks pass), the scratch size, the ValueErrors
of ops.gat_aggregate(schedule="flat"), and the fp32 numpy emulation of the rule (tests/_gat_flat_ref.py: per-chunk running
states merged in chunk order) inside the float64 bound of _gat_ref.forward on every graph x mask of the GPU test, at the
library's T = 256 and at T = 128 -- the bound can be met by the rule itself."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import _gat_flat_ref as R
import _gat_ref as G

OK, NULL, SHAPE, UNSUPPORTED, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -7
F16, F32 = 0, 1


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_symbols(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    for name in ("sgx_gat_flat_scratch_bytes", "sgx_gat_aggregate_flat"):
        assert name in L.SYMBOLS and f" T {name}\n" in out
    fn = L.lib.sgx_gat_aggregate_flat
    assert fn.restype == i
    assert list(fn.argtypes) == [i, i, i, i, i, i, f, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, vp, ctypes.c_size_t,
                                 ctypes.POINTER(L.GatStats), vp]
    size = L.lib.sgx_gat_flat_scratch_bytes
    assert (size.restype, list(size.argtypes)) == (ctypes.c_size_t, [i64, i, i, i, i])
    assert L.lib.sgx_spmm_flat_chunk() == 256


def test_scratch_bytes(L):
    T, size = L.lib.sgx_spmm_flat_chunk(), L.lib.sgx_gat_flat_scratch_bytes
    assert size(-1, 10, 10, 64, 0) == 0 and size(1 << 31, 10, 10, 64, 0) == 0 and size(10, -1, 10, 64, 0) == 0
    assert size(10, 11, 10, 64, 0) == 0 and size(10, 10, 10, 0, 0) == 0
    for n_feat in (1, 3, 64, 100):
        for mean in (0, 1):
            last = 0
            for nnz in (0, 1, T - 1, T, T + 1, 3 * T, 10 * T + 5, 1 << 20):
                b = size(nnz, 50, 60, n_feat, mean)
                assert b >= last and b > 0 and b % 256 == 0, (nnz, n_feat, mean)
                last = b
            # one chunk more (regions are rounded up to 256 bytes: visible once two states of a chunk fill one)
            assert n_feat < 64 or size(T + 1, 50, 60, n_feat, mean) > size(T, 50, 60, n_feat, mean)
            # two states per chunk: n_feat floats of acc and (m, l), and the chunk's meta
            chunks = 10 * T // T + 1
            assert size(10 * T + 5, 50, 60, n_feat, mean) >= chunks * 2 * (n_feat + 2) * 4 + chunks * 8 + 2 * 60 * 4
        assert size(100, 50, 60, n_feat, 1) >= size(100, 50, 60, n_feat, 0) + n_feat * 4      # the mean row and its slabs


def _call(L, **kw):
    a = dict(dtype=F16, relu=0, n_rows=50, n_cols=100, n_feat=64, n_heads=1, alpha=0.2, nnz=1000, rowPtr=0x10000,
             columnIndex=0x20000, values=0x30000, Wh=0x40000, ldh=64, attention=0x48000, D=0x50000, ldd=64, fill=None, n_nodes=0,
             scratch=0x60000, scratch_bytes=None, stats=None, stream=None)
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = L.lib.sgx_gat_flat_scratch_bytes(max(a["nnz"], 0), max(a["n_rows"], 0), max(a["n_cols"], a["n_rows"], 0),
                                                              max(a["n_feat"], 1), int(a["fill"] is None and a["n_nodes"] != 0))
    return L.lib.sgx_gat_aggregate_flat(*a.values())


def test_argument_errors_need_no_gpu(L):
    # those of sgx_spmm_csr_flat
    for kw in (dict(n_rows=-1), dict(n_cols=-1), dict(n_cols=49), dict(n_feat=0), dict(ldh=63), dict(ldd=63), dict(nnz=-1),
               dict(nnz=1 << 31)):
        assert _call(L, **kw) == SHAPE, kw
    assert _call(L, dtype=2) == UNSUPPORTED
    assert _call(L, n_rows=0, rowPtr=None, D=None) == OK                 # nothing to store: nothing is looked at
    for kw in (dict(rowPtr=None), dict(D=None), dict(columnIndex=None), dict(values=None), dict(Wh=None), dict(attention=None)):
        assert _call(L, **kw) == NULL, kw
    assert _call(L, nnz=0, columnIndex=None, values=None, scratch=None) == WORKSPACE       # what nnz == 0 excuses
    assert _call(L, n_cols=1 << 25, ldh=64) == UNSUPPORTED               # 2^25 x 64 x 2 bytes = 4 GiB
    assert _call(L, dtype=F32, n_cols=1 << 24, ldh=64) == UNSUPPORTED
    assert _call(L, n_feat=1 << 19, ldh=1 << 19, ldd=1 << 19, n_rows=1, n_cols=2) == UNSUPPORTED
    assert _call(L, scratch=None) == WORKSPACE
    assert _call(L, scratch_bytes=L.lib.sgx_gat_flat_scratch_bytes(1000, 50, 100, 64, 0) - 1) == WORKSPACE
    assert _call(L, nnz=1025, scratch_bytes=L.lib.sgx_gat_flat_scratch_bytes(1024, 50, 100, 64, 0)) == WORKSPACE   # one chunk more
    assert _call(L, n_nodes=100, scratch_bytes=L.lib.sgx_gat_flat_scratch_bytes(1000, 50, 100, 64, 0)) == WORKSPACE  # the mean row
    for kw in (dict(scratch=0x60000 + 128), dict(rowPtr=0x10002), dict(columnIndex=0x20002), dict(values=0x30001), dict(Wh=0x40001),
               dict(attention=0x48001), dict(D=0x50001), dict(fill=0x70002, n_nodes=7), dict(dtype=F32, values=0x30002),
               dict(dtype=F32, Wh=0x40002), dict(dtype=F32, D=0x50002)):
        assert _call(L, **kw) == ALIGN, kw
    # one head only
    for heads in (2, 8):
        assert _call(L, n_heads=heads) == UNSUPPORTED
    assert _call(L, n_heads=0, scratch=None) == WORKSPACE                # 0 counts as one head: the error behind it
    # those of sgx_gat_aggregate_stats: the dead-row rule and the statistics
    for kw in (dict(n_nodes=99), dict(n_nodes=-1), dict(fill=0x70000, n_nodes=0), dict(fill=0x70000, n_nodes=1 << 31)):
        assert _call(L, **kw) == SHAPE, kw
    assert _call(L, n_nodes=100, scratch=None) == WORKSPACE and _call(L, fill=0x70000, n_nodes=7, scratch=None) == WORKSPACE
    full = dict(score_row=0x80000, score_col=0x81000, row_max=0x82000, row_sum=0x83000)
    for missing in full:
        st = L.GatStats(**{**full, missing: None})
        assert _call(L, stats=ctypes.byref(st)) == NULL, missing
    st = L.GatStats(**full)
    assert _call(L, stats=ctypes.byref(st), scratch=None) == WORKSPACE   # complete statistics pass; NULL statistics are allowed


def test_ops_value_errors(L):
    from sgracex1_amd import ops
    A = ops.Csr.__new__(ops.Csr)                                         # the facts alone: no device tensors here
    A._plan, A._max_row, A._flat, A._nnz = None, None, False, 10
    Wh, att = torch.zeros(4, 8), torch.zeros(16)
    with pytest.raises(ValueError, match="schedule must be None or 'flat'"):
        ops.gat_aggregate(A, Wh, att, schedule="rows")
    with pytest.raises(ValueError, match="one head and no edge outputs"):
        ops.gat_aggregate(A, Wh, att, schedule="flat", want_edge_outputs=True)
    with pytest.raises(ValueError, match="one head and no edge outputs"):
        ops.gat_aggregate(A, Wh, att, schedule="flat", heads=2)


CPU_WIDTH = 8


@pytest.mark.parametrize("T", [256, 128])
def test_emulated_rule_lies_inside_the_float64_bound(L, T):
    """per-chunk running states merged in chunk order, in fp32, against _gat_ref.forward: every graph x mask, both storage
    types, the three dead rules (the activation alternating), at the library's T and at another"""
    if T == 256:
        assert L.lib.sgx_spmm_flat_chunk() == T
    crossing = merged_dead = 0
    for name in R.degree_cases(T):
        for mask in R.MASKS:
            for dt in ("f16", "f32"):
                g = R.graph(name, mask, CPU_WIDTH, dt, T)
                for k, rule in enumerate(("zero", "mean", "fill")):
                    relu = (k + len(name)) % 2
                    ref = R.reference(g, dt, relu, rule)
                    got, dead = R.emulate(g, T, relu, rule, dt)
                    assert (dead == ref["dead"]).all(), (name, mask, dt)
                    G.check(f"{name} {mask} {dt} {rule} T={T}", got, ref["D"], ref["bD"], np.arange(g["n_rows"]), {})
                if dt == "f16" and mask == "chunks":
                    rp = g["rowptr"]
                    cross = (np.diff(rp) > 0) & (rp[:-1] // T != (np.maximum(rp[1:], 1) - 1) // T)
                    crossing += int(cross.sum())
                    merged_dead += int((cross & ref["dead"]).sum())
    assert crossing >= 8 and merged_dead >= 1


def test_masks_are_what_they_say(L):
    T = 256
    g = R.graph("masked_chunks", "chunks", 8, "f16", T)
    rp, live = g["rowptr"], g["val"] > 0
    chunk = np.arange(rp[-1]) // T
    assert rp[1] // T == 0 and (rp[2] - 1) // T == 3                     # row 1 leads from chunk 0 and reaches chunk 3
    assert not live[rp[1]:rp[2]][chunk[rp[1]:rp[2]] % 2 == 0].any() and live[rp[1]:rp[2]][chunk[rp[1]:rp[2]] == 1].all()
    assert (rp[4] - 1) // T - rp[3] // T >= 3 and not live[rp[3]:rp[4]].any()      # row 3: dead over four chunks
    third = R.graph("mixed", "third", 8, "f32", T)["val"]
    assert 0.2 < (third <= 0).mean() < 0.45 and np.signbit(third[third == 0]).any() and (~np.signbit(third[third == 0])).any()
    assert ((third > 0) & (third < 2.0 ** -126)).any() and (third < 0).any()
    for mask, sign in (("ascend", 1), ("descend", -1)):
        g = R.graph("long_leading", mask, 8, "f32", T)
        E = R.reference(g, "f32", 0, "zero")["E"]
        mean = [E[k * T:(k + 1) * T].mean() for k in range(5)]
        assert all(3.0 < sign * (b - a) < 5.0 for a, b in zip(mean, mean[1:])), (mask, mean)
