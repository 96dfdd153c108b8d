"""The sampler's wide form without a GPU: its numpy restatement (tests/_sampler_wide_ref.py) against Floyd's sequential
loop (_sampler_ref.floyd), and the host queries sgx_sample_form / sgx_sample_wide_max with their Python names."""
import os
import re
import subprocess

import numpy as np
import pytest

import _sampler_ref as R
import _sampler_wide_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = -2

KS = (65, 100, 127, 128, 129, 255, 1023, 1024)
GRID = [(k, deg) for k in KS for deg in (k + 1, k + 2, k + 7, 2 * k, 3 * k + 1, 70001)]
DENSE = [(k, k + 1) for k in range(65, 131)]               # nearly every draw collides: long chains


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _keys(n, seed):
    return [int(x) for x in np.random.default_rng(seed).integers(0, 2 ** 63, n)]


def test_restatement_equals_floyd_on_the_grid():
    for (k, deg), key0 in zip(GRID, _keys(len(GRID), 0)):
        for v in range(12):
            assert W.wide(key0 + v, v, deg, k) == R.floyd(key0 + v, v, deg, k), (k, deg, v)


def test_restatement_equals_floyd_on_dense_hits_with_long_chains():
    longest, hits = 0, 0
    for (k, deg), key in zip(DENSE, _keys(len(DENSE), 1)):
        for v in (0, 3, 2_000_000):
            assert W.wide(key, v, deg, k) == R.floyd(key, v, deg, k), (k, deg, v)
            dup, par = W.chain_words(R.draws(key, v, deg, k), deg - k)
            hit, _ = W.jump(dup, par)
            longest = max(longest, W.chain_length(par))
            hits += int(hit.sum()) - int(dup.sum())         # hits that only the chain gives
    assert longest >= 3, longest                            # some chain needs more than one jump
    assert hits > 0


def test_rounds_and_chunked_jumping():
    assert [W.rounds_of(k) for k in (2, 3, 4, 65, 128, 129, 1024)] == [1, 2, 2, 7, 7, 8, 10]
    # the longest chain there is: every element hangs on the one before it, only the root is a duplicate
    for k in (65, 128, 129, 1024):
        dup = np.zeros(k, bool)
        dup[0] = True
        hit, par = W.jump(dup, np.arange(-1, k - 1))
        assert hit.all() and (par < 0).all()
        hit, _ = W.jump(np.zeros(k, bool), np.arange(-1, k - 1))
        assert not hit.any()


def test_form_and_cut_through_the_abi(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_sample_form", "sgx_sample_wide_max"):
        assert name in L.SYMBOLS and f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110
    assert L.lib.sgx_sample_wide_max() == 1024
    form = L.lib.sgx_sample_form
    assert [form(k) for k in (-2, -1, 0, 64, 65, 1024, 1025)] == [SHAPE, 0, 1, 1, 2, 2, 3]
    assert form(-(2 ** 31)) == SHAPE and form(2 ** 31 - 1) == 3


def test_form_in_python(L):
    from sgracex1_amd import ops
    assert ops.SAMPLE_WIDE_MAX == 1024
    assert [ops.sample_form(k) for k in (-1, 0, 64, 65, 1024, 1025)] == [0, 1, 1, 2, 2, 3]
    assert ops.sample_form(ops.SAMPLE_WIDE_MAX) == 2 and ops.sample_form(ops.SAMPLE_WIDE_MAX + 1) == 3
    with pytest.raises(ValueError):
        ops.sample_form(-2)


def test_header_declares_what_is_bound(L):
    text = open(L.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in L.SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(L.lib, name), name
    assert re.search(r"\bint\s+sgx_sample_wide_max\s*\(\s*void\s*\)\s*;", code)
    assert re.search(r"\bint\s+sgx_sample_form\s*\(\s*int\s+fanout\s*\)\s*;", code)
    # the sampler's other signatures are as they were
    assert L.ABI.functions["sgx_sample_workspace_bytes"][1] == L.ABI.functions["sgx_node_batch_workspace_bytes"][1]
    assert len(L.ABI.functions["sgx_sample_neighbors"][1]) == 22
    assert "larger ones are correct and slow" not in text
