"""The restatement of sgx_xt_g's host side (tests/_xtg_ref.py) without a GPU: geometry() pinned for every row of the shape
table the GPU tests run (tests/test_gpu_xt_g_arms.py), the arm and arrangement each row is meant to reach, and the table's
coverage -- all eight xtg_partial_wg_kernel<TX, WM, WP> instantiations plus the wave and the scalar kernel -- so that a
change to the table or to the dispatch rule cannot quietly stop an arm from being tested.  The library's
sgx_xt_g_workspace_bytes is a host function: it is held to the restatement here as well."""
import pytest
import torch

import _xtg_ref as R

IDS = [f"{n}x{M}x{P}" for n, M, P, *_ in R.SHAPES]


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


@pytest.mark.parametrize("n,M,P,arm,arr,why", R.SHAPES, ids=IDS)
def test_geometry_pinned(n, M, P, arm, arr, why):
    assert R.geometry(n, M, P) == R.GEOMETRY[(n, M, P)]
    n_slabs, rps, m_pad, p_pad, wm = R.geometry(n, M, P)
    assert rps % 16 == 0 and n_slabs * rps >= n and (n_slabs - 1) * rps < max(n, 1)       # the slabs cover the rows, none is empty
    assert m_pad % 64 == 0 and 0 <= m_pad - M < 64 and p_pad % 64 == 0 and 0 <= p_pad - P < 64
    assert R.arrangement(n, M, P) == arr
    for dt in R.DTYPES:
        assert R.arm(n, dt, R.padded_ld(M), P + 3) == arm     # the padded views of the mask test
        odd_half = dt == torch.float16 and M % 2 == 1 and n > 0
        assert R.arm(n, dt, M, P) == ("scalar" if odd_half else arm)           # contiguous: odd fp16 rows are not dword-aligned


def test_arm_rule():
    h, f = torch.float16, torch.float32
    n = R.WG_MIN_ROWS
    assert R.arm(n, h, 64, 64) == "wg" and R.arm(n - 1, h, 64, 64) == "vec" and R.arm(0, h, 64, 64) == "zero"
    assert R.arm(n, h, 64, 64, wave_tiles_override=True) == "vec"
    assert R.arm(n, h, 64, 64, scalar_override=True) == "scalar"
    assert R.arm(n, f, 64, 64, scalar_override=True, wave_tiles_override=True) == "scalar"
    # rows that are not dword-aligned: an odd pitch or an odd element address in fp16 only
    assert R.arm(n, h, 65, 64) == "scalar" and R.arm(n, f, 65, 64) == "wg" and R.arm(n, h, 66, 64) == "wg"
    assert R.arm(n, h, 64, 64, x_addr=2) == "scalar" and R.arm(100, h, 64, 64, x_addr=4098) == "scalar"
    assert R.arm(n, f, 64, 64, x_addr=4) == "wg" and R.arm(n, f, 64, 64, g_addr=4) == "wg"
    # tables whose byte offsets do not fit 32 bits
    assert R.arm(1 << 24, f, 64, 64) == "scalar" and R.arm(1 << 24, h, 64, 8) == "wg" and R.arm(1 << 24, h, 64, 64) == "scalar"


def test_table_covers_every_arm():
    # (derived from the restatement alone; tests/test_gpu_xt_g_arms.py asserts the same rule on the real address and pitch
    # of every operand it launches with, and the workspace test below ties geometry() to the library)
    reached = set()
    for n, M, P, arm, arr, why in R.SHAPES:
        for dt in R.DTYPES:
            name = {torch.float16: "f16", torch.float32: "f32"}[dt]
            a = R.arm(n, dt, R.padded_ld(M), P + 3)
            reached.add((name, R.arrangement(n, M, P)) if a == "wg" else (name, a))
            if n > 0:
                # what the GPU test reaches on the same shape: the overrides, and fp16 rows that are not dword-aligned
                reached.add((name, R.arm(n, dt, R.padded_ld(M), P, wave_tiles_override=True)))
                reached.add((name, R.arm(n, dt, M, P, scalar_override=True)))
                if dt == torch.float16:
                    assert R.arm(n, dt, R.padded_ld(M) + 1, P) == "scalar" and R.arm(n, dt, R.padded_ld(M), P, x_addr=2) == "scalar"
    want = {(t, a) for t in ("f16", "f32") for a in ("8x1", "4x2", "2x4", "1x8", "vec", "scalar", "zero")}
    assert reached == want
    # every row count the table promises, and every arrangement at the threshold itself
    counts = {n for n, *_ in R.SHAPES}
    assert {0, 1, 3, 63, 64, 65, 1000, R.N0 - 1, R.N0, R.N0 + 1, R.N0 + 37} == counts
    assert {arr for n, M, P, arm, arr, why in R.SHAPES if n == R.N0} == {"8x1", "4x2", "2x4", "1x8"}


@pytest.mark.parametrize("n,M,P,arm,arr,why", R.SHAPES, ids=IDS)
def test_library_workspace_matches_restatement(L, n, M, P, arm, arr, why):
    n_slabs, rps, m_pad, p_pad, wm = R.geometry(n, M, P)
    assert L.lib.sgx_xt_g_workspace_bytes(n, M, P) == R.align256(n_slabs * m_pad * p_pad * 4) == R.workspace_bytes(n, M, P)


def test_library_workspace_edges(L):
    """n_rows = 0 is a valid call and returns one 64 x 64 tile per tile of the output; bad shapes give 0; the 64 MiB cap on
    the partial products bounds the slab count of a wide product."""
    ws = L.lib.sgx_xt_g_workspace_bytes
    assert ws(0, 1, 1) == 64 * 64 * 4 == R.workspace_bytes(0, 1, 1)
    assert ws(-1, 64, 64) == 0 and ws(10, 0, 64) == 0 and ws(10, 64, 0) == 0
    for n, M, P in [(1 << 20, 1433, 512), (1 << 20, 4096, 4096), (100003, 64, 64), (40001, 602, 128), (9000, 128, 256)]:
        assert ws(n, M, P) == R.workspace_bytes(n, M, P)
        assert R.workspace_bytes(n, M, P) <= 64 << 20 or R.geometry(n, M, P)[0] == 1
