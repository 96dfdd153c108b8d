"""Model selection without a GPU: the numpy restatement of sgx_keep_best's rule on a sequence worked out by hand, the new
symbol and the layout of its structs against the C compiler, every argument error of the call on made-up addresses, and
the host checks of ops.keep_best."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _keep_best_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, UNSUPPORTED, ALIGN = -1, -2, -3, -7


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_restatement_on_the_hand_sequence():
    """Validates the REFERENCE: 0/5, 1/3, 2/6, 2/5, 2/5, 1/2, n = 0, hits > n, n = 2^31 -> the best epochs are 1, then 3,
    then 5; a tie and an out-of-range candidate leave everything but `epoch` alone."""
    state = R.fresh_state()
    src, dst = np.zeros(5, np.uint32), np.full(5, 77, np.uint32)
    log = np.full((len(R.SEQUENCE) - 2, 6), -1, np.int64)              # two rows short of the calls
    wins = []
    for e, (n, hits) in enumerate(R.SEQUENCE):
        src[:] = 0x7FC00000 + e                                        # NaN payloads: the copy is of bits
        before, kept = state.copy(), dst.copy()
        sums = [np.array([n, hits, 1000 + e], np.int64), np.array([7, e, -e], np.int64)]
        won = R.keep_best([src], [dst], sums, state, log)
        wins.append(won)
        assert state[3] == e + 1 and state[2] == R.BEST_AFTER[e]
        if won:
            assert tuple(state[:3]) == (n, hits, e) and (dst == src).all()
        else:
            assert (state[:3] == before[:3]).all() and (dst == kept).all()
        if e < log.shape[0]:
            assert list(log[e]) == [n, hits, 1000 + e, 7, e, -e]
    assert [e for e, w in enumerate(wins) if w] == [1, 3, 5]
    assert tuple(state) == (2, 1, 5, len(R.SEQUENCE)) and (dst == 0x7FC00000 + 5).all()
    assert (log[:, 2] == 1000 + np.arange(log.shape[0])).all()       # every row written once, none past the end
    # the comparison is cross-multiplied, not divided: 1/3 against 333333333/10^9 differ in the tenth digit only
    assert R.better(3, 1, 10 ** 9, 333333333) and not R.better(10 ** 9, 333333333, 3, 1)
    assert not R.better(5, 2, 1 << 31, 0) and not R.better(5, -1, 1, 0) and R.better((1 << 31) - 1, 1, 1, 0)


def test_symbol_and_struct_layout(L, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    assert "sgx_keep_best" in L.SYMBOLS and " T sgx_keep_best\n" in out
    assert L.lib.sgx_version() == 110
    assert (L.SGX_BEST_MAX_TENSORS, L.SGX_BEST_MAX_SUMS) == (L.SGX_ADAM_MAX_TENSORS, 4) == (16, 4)
    vp = ctypes.c_void_p
    assert L.BestTensor._fields_ == [("src", vp), ("dst", vp), ("n", ctypes.c_int64)]
    assert L.BestDesc._fields_ == [("n_tensors", ctypes.c_int32), ("n_sums", ctypes.c_int32), ("sums", vp * 4), ("state", vp),
                                   ("log", vp), ("log_rows", ctypes.c_int64), ("tensor", L.BestTensor * 16)]
    fn = L.lib.sgx_keep_best
    assert (fn.restype, list(fn.argtypes)) == (ctypes.c_int, [ctypes.POINTER(L.BestDesc), vp])
    lines = []
    for c_name, cls in (("sgx_best_tensor", L.BestTensor), ("sgx_best_desc", L.BestDesc)):
        lines.append(f' printf("{c_name} %zu\\n", sizeof({c_name}));\n')
        lines += [f' printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));\n' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n' + "".join(lines) + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    said = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())}
    for c_name, cls in (("sgx_best_tensor", L.BestTensor), ("sgx_best_desc", L.BestDesc)):
        assert said[c_name] == ctypes.sizeof(cls)
        for f, _ in cls._fields_:
            assert said[f"{c_name}.{f}"] == getattr(cls, f).offset, (c_name, f)


def _desc(L, n_tensors=2, n_sums=2, log_rows=3):
    d = L.BestDesc()
    d.n_tensors, d.n_sums = n_tensors, n_sums
    for k in range(n_sums):
        d.sums[k] = 256 * (k + 1)
    d.state, d.log, d.log_rows = 4096, 8192, log_rows
    for k in range(n_tensors):
        d.tensor[k].src, d.tensor[k].dst, d.tensor[k].n = 65536 * (k + 1), 65536 * (k + 1) + 32768, 10
    return d


def test_argument_errors_need_no_gpu(L):
    run = lambda d: L.lib.sgx_keep_best(None if d is None else ctypes.byref(d), None)
    assert run(None) == NULL
    d = _desc(L)
    d.state = None
    assert run(d) == NULL
    for k in range(2):
        d = _desc(L)
        d.sums[k] = None
        assert run(d) == NULL, k
    for field in ("src", "dst"):
        d = _desc(L)
        setattr(d.tensor[1], field, None)
        assert run(d) == NULL, field
    for n_tensors in (-1, L.SGX_BEST_MAX_TENSORS + 1):
        d = _desc(L)
        d.n_tensors = n_tensors
        assert run(d) == SHAPE, n_tensors
    for n_sums in (0, -1, L.SGX_BEST_MAX_SUMS + 1):
        d = _desc(L)
        d.n_sums = n_sums
        assert run(d) == SHAPE, n_sums
    d = _desc(L)
    d.tensor[0].n = -1
    assert run(d) == SHAPE
    d = _desc(L)
    d.log_rows = -1
    assert run(d) == SHAPE
    d = _desc(L)
    d.log = None
    assert run(d) == NULL                               # log NULL with log_rows > 0
    d = _desc(L)
    d.tensor[1].dst = d.tensor[1].src
    assert run(d) == UNSUPPORTED
    d = _desc(L)
    d.tensor[0].src = d.tensor[0].src + 2
    assert run(d) == ALIGN
    # what n == 0 excuses: NULL and equal pointers on a skipped tensor are never looked at -- shown by the error behind them
    d = _desc(L)
    d.tensor[0].n, d.tensor[0].src, d.tensor[0].dst = 0, None, None
    d.tensor[1].dst = d.tensor[1].src
    assert run(d) == UNSUPPORTED


def test_ops_keep_best_host_checks(L):
    from sgracex1_amd import ops
    f = lambda n=4: torch.zeros(n)
    state, sums = torch.tensor([1, 0, -1, 0]), [torch.zeros(3, dtype=torch.int64)]
    with pytest.raises(ValueError, match="one snapshot"):
        ops.keep_best([f()], [], sums, state)
    with pytest.raises(ValueError, match="at most 16"):
        ops.keep_best([f()] * 17, [f()] * 17, sums, state)
    for bad in ([], sums * 5):
        with pytest.raises(ValueError, match="1 to 4 sums"):
            ops.keep_best([f()], [f()], bad, state)
    with pytest.raises(ValueError, match="state must be a tensor on the GPU"):
        ops.keep_best([f()], [f()], sums, state)         # host tensors are refused before anything is dereferenced
    with pytest.raises(ValueError, match="state must be a tensor on the GPU"):
        ops.keep_best([f()], [f()], sums, [1, 0, -1, 0])


def test_tracker_refuses_more_than_sixteen_tensors(L):
    from sgracex1_amd.train import BestTracker
    trainer = type("T", (), {"params": [torch.zeros(1)] * 17, "model": None})()
    with pytest.raises(ValueError, match="at most 16"):
        BestTracker(trainer)
