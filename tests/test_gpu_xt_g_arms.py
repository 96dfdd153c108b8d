"""X^T . G (sgx_xt_g) on every kernel the entry point can launch, at the shapes of tests/_xtg_ref.py: the four WM x WP
arrangements of the workgroup kernel for fp16 and fp32 X, the wavefront-tile kernel and the scalar kernel.

Every case checks
  value   |got - X64^T G64| / (|X|64^T |G|64) < 5e-6 elementwise (the bound of test_xt_g_matches_fp64, unchanged);
  bits    the same result from every kernel that can run the shape: SGX_XTG_WAVE_TILES, SGX_XTG_SCALAR, and -- fp16 --
          the scalar kernel reached without an override, through an X whose address is 2 mod 4 and through an odd pitch;
  masks   X and G as views into larger buffers (ldx > M, ldg > P, rows before and after the n rows used) whose pad
          columns and outside rows hold NaN in one run and 1e30 in another: bit-equal to the contiguous run.  The pitch of
          X stays even, so that fp16 rows keep the 16-byte-load kernels: 602 -> 604 and 7 -> 8 put a 4-wide chunk across M.
"""
import ctypes

import pytest
import torch

import _xtg_ref as R

pytestmark = pytest.mark.gpu

BOUND = 5e-6
ROWS_BEFORE, ROWS_AFTER = 3, 5
IDS = [f"{n}x{M}x{P}" for n, M, P, *_ in R.SHAPES]


def _operands(n, M, P, xdtype):
    g = torch.Generator(device="cuda")
    g.manual_seed(1000003 * n + 1009 * M + P)
    X = torch.randn((n, M), generator=g, device="cuda").to(xdtype)
    G = torch.randn((n, P), generator=g, device="cuda")
    return X, G


def _view(t, ld, fill, before=ROWS_BEFORE, after=ROWS_AFTER, skip=0):
    """t's values as a view of pitch ld into a buffer filled with `fill`, `before` / `after` rows around it; skip: elements
    the view's address lies past the buffer's (1: an fp16 view that is not dword-aligned)."""
    n, w = t.shape
    buf = torch.full(((before + n + after) * ld + skip,), fill, dtype=torch.float32, device=t.device).to(t.dtype)   # (1e30: inf as fp16)
    v = buf[skip:].view(before + n + after, ld)[before:before + n, :w]
    v.copy_(t)
    assert v.stride(0) == ld and v.data_ptr() == buf.data_ptr() + (skip + before * ld) * t.element_size()
    return v


def _arm(X, G, **kw):
    return R.arm(X.shape[0], X.dtype, X.stride(0), G.stride(0), X.data_ptr(), G.data_ptr(), **kw)


@pytest.mark.parametrize("xdtype", R.DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("n,M,P,arm,arr,why", R.SHAPES, ids=IDS)
def test_xt_g_every_arm(n, M, P, arm, arr, why, xdtype):
    from sgracex1_amd import _lib, ops
    X, G = _operands(n, M, P, xdtype)
    got = ops.xt_g(X, G)
    assert got.shape == (M, P) and got.dtype == torch.float32
    if n == 0:
        assert torch.equal(got, torch.zeros_like(got))              # (NULL operands: test_xt_g_leaves_out_pad_columns)
        for override in ("SGX_XTG_WAVE_TILES", "SGX_XTG_SCALAR"):
            with _lib.tuning(**{override: "1"}):
                assert torch.equal(ops.xt_g(X, G), got), override
        return

    # value
    want = X.double().t() @ G.double()
    scale = X.double().abs().t() @ G.double().abs()
    err = ((got.double() - want).abs() / scale).max().item()
    print(f"xt_g {n}x{M}x{P} {xdtype}: max |err| / (|X|^T |G|) = {err:.3e} (bound {BOUND:.0e})")
    assert err < BOUND

    # the same bits on every kernel that can run the shape
    odd_half = xdtype == torch.float16 and M % 2 == 1
    assert _arm(X, G) == ("scalar" if odd_half else arm)
    with _lib.tuning(SGX_XTG_WAVE_TILES="1"):
        assert torch.equal(ops.xt_g(X, G), got), "SGX_XTG_WAVE_TILES"
    with _lib.tuning(SGX_XTG_SCALAR="1"):
        assert torch.equal(ops.xt_g(X, G), got), "SGX_XTG_SCALAR"
    nan = float("nan")
    if xdtype == torch.float16:
        Xo = _view(X, R.padded_ld(M), nan, skip=1)
        assert Xo.data_ptr() % 4 == 2 and Xo.stride(0) % 2 == 0 and _arm(Xo, G) == "scalar"
        assert torch.equal(ops.xt_g(Xo, G), got), "X at an address that is 2 mod 4"
        Xo = _view(X, R.padded_ld(M) + 1, nan, before=2)
        assert Xo.data_ptr() % 4 == 0 and Xo.stride(0) % 2 == 1 and _arm(Xo, G) == "scalar"
        assert torch.equal(ops.xt_g(Xo, G), got), "X with an odd pitch"

    # masks: pad columns and rows outside the table never reach a sum
    for fill in (nan, 1e30):
        Xv, Gv = _view(X, R.padded_ld(M), fill), _view(G, P + 3, fill)
        assert _arm(Xv, Gv) == arm
        assert torch.equal(ops.xt_g(Xv, Gv), got), f"padded views filled with {fill}"
        with _lib.tuning(SGX_XTG_WAVE_TILES="1"):
            assert torch.equal(ops.xt_g(Xv, Gv), got), f"padded views filled with {fill}, SGX_XTG_WAVE_TILES"


def test_workspace_bytes_match_restatement():
    from sgracex1_amd._lib import lib
    for n, M, P, *_ in R.SHAPES:
        n_slabs, rps, m_pad, p_pad, wm = R.geometry(n, M, P)
        assert lib.sgx_xt_g_workspace_bytes(n, M, P) == R.align256(n_slabs * m_pad * p_pad * 4), (n, M, P)


@pytest.mark.parametrize("n,M,P", [(R.N0, 7, 300), (1000, 602, 128), (0, 64, 64)])
def test_xt_g_leaves_out_pad_columns(n, M, P):
    """include/sgx.h: columns P .. ldo-1 of out are not written.  Without rows X and G may be NULL and out is cleared."""
    from sgracex1_amd import ops
    from sgracex1_amd._lib import SGX_F32, lib
    X, G = _operands(n, M, P, torch.float32)
    want = ops.xt_g(X, G)
    ldo, sentinel = P + 5, -12345.5
    out = torch.full((M, ldo), sentinel, device="cuda")
    ws = torch.empty(max(lib.sgx_xt_g_workspace_bytes(n, M, P), 256), dtype=torch.uint8, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    rc = lib.sgx_xt_g(SGX_F32, n, M, P, vp(X), M, vp(G), P, vp(out), ldo, vp(ws), ws.numel(),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert torch.equal(out[:, :P], want)
    assert torch.equal(out[:, P:], torch.full((M, ldo - P), sentinel, device="cuda"))
