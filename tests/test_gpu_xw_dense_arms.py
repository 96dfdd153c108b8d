"""Dense X.W (sgx_xw_dense) on every kernel arm the entry point dispatches to, at the cases of tests/_xw_dense_ref.py.

Every case first asserts WHICH kernel runs -- ops.xw_dense_form (sgx_xw_dense_form, answered by the functions the launch
uses): kind, template arguments, column blocks, max_trips -- and then checks
  value   every element against X.double() @ Wt.double().t() within (M + 2) 2^-24 (|X| |W|) + one store rounding; the case
          prints max err / bound;
  bits    the same bits as the tile kernel, reached without an override on row chunks of 4096 (under every gate), and as
          every arm an override leads to (SGX_XW_NO_WLDS, SGX_XW_NO_STATIONARY_F32, SGX_XW_NO_LDS, SGX_XW_SHORT_TILES);
  relu    relu=True == where(got > 0, got, +0) bit for bit;
  pads    columns P .. ldh-1 are exact zeros.
Then, one case per kind and dtype: masks (operands as views into buffers of NaN / 1e30), guard bands around out= at four
alignments, hostile values (NaN rows, +-inf at a row's first and last k, a NaN row of Wt).
"""
import functools

import pytest
import torch

import _xw_dense_ref as D

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"f16": torch.float16, "f32": torch.float32}
IDS = [c.name for c in D.CASES]
NAN = float("nan")


@functools.lru_cache(maxsize=2)
def _operands(n, M, P, dt):
    X, Wt = D.operands(n, M, P, dt)
    return torch.from_numpy(X).cuda(), torch.from_numpy(Wt).cuda()


def _view(t, ld, skip=0, fill=0.0, before=0, after=0):
    """t's values as a view of pitch ld into a buffer filled with `fill`, `before` / `after` rows around it, the view's
    address `skip` elements past a 256-byte aligned one"""
    n, w = t.shape
    buf = torch.full((skip + (before + n + after) * ld,), fill, dtype=torch.float32, device=t.device).to(t.dtype)   # (1e30: inf as fp16)
    v = buf[skip:].view(before + n + after, ld)[before:before + n, :w]
    v.copy_(t)
    assert (n <= 1 or v.stride(0) == ld) and v.data_ptr() == buf.data_ptr() + (skip + before * ld) * t.element_size()
    return v


def _out(case, n, P, ldh, skip, fill=0.0, before=0, after=0):
    """(buffer, out= view [n, P] of row stride ldh) for xw_dense"""
    buf = torch.full((skip + (before + n + after) * ldh,), fill, dtype=TORCH_DTYPE[case.dt], device="cuda")
    out = torch.as_strided(buf, (n, P), (ldh, 1), skip + before * ldh)
    return buf, out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _laid_out(case, X, Wt):
    ldx, xs, ldw, ws = D.layout(case)[:4]
    return (_view(X, ldx, xs) if case.x else X), (_view(Wt, ldw, ws) if case.w else Wt)


def _run(case, Xv, Wv, relu=False, want_form=False):
    """xw_dense as the case lays H out (out= where the case says so): (result [n, P], all ldh columns [n, ldh], form)"""
    from sgracex1_amd import ops
    ldh, hs = D.layout(case)[4:]
    n, P = Xv.shape[0], Wv.shape[0]
    if case.h:
        _, out = _out(case, n, P, ldh, hs, fill=NAN)
        kw = dict(out=out)
    else:
        kw = dict(ldh=case.ldh)
    form = ops.xw_dense_form(Xv, Wv, **kw) if want_form else None
    got = ops.xw_dense(Xv, Wv, relu=relu, **kw)
    full = torch.as_strided(got, (n, ldh), (ldh, 1)) if n else got
    return got, full, form


def _tile_reference(case, Xv, Wv):
    """the tile kernel's result, without an override: row chunks under every gate"""
    from sgracex1_amd import ops
    parts = []
    for r in range(0, Xv.shape[0], D.CHUNK):
        chunk = Xv[r:r + D.CHUNK]
        assert ops.xw_dense_form(chunk, Wv).kind == "tile"
        parts.append(ops.xw_dense(chunk, Wv))
    return torch.cat(parts)


def _bound(X, Wt, dt):
    """(want, bound) in float64 on the device: D.bound, the expression the CPU test shows to have no slack"""
    want = X.double() @ Wt.double().t()
    return want, D.bound(X.shape[1], X.double().abs() @ Wt.double().abs().t(), want, dt)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_xw_dense_every_arm(case):
    from sgracex1_amd import _lib
    X, Wt = _operands(case.n, case.M, case.P, case.dt)
    Xv, Wv = _laid_out(case, X, Wt)
    env = {k: "1" for k in case.env}
    with _lib.tuning(**env):
        got, full, f = _run(case, Xv, Wv, want_form=True)
        act, act_full, _ = _run(case, Xv, Wv, relu=True)
    assert (f.kind, f.a, f.b) == case.arm and f.blocks == case.blocks and f.max_trips >= case.trips, f
    assert f.vec and (case.wgs is None or f.wgs_per_cu == case.wgs), f

    # value
    want, bound = _bound(X, Wt, case.dt)
    ratio = ((got.double() - want).abs() / bound).max().item()
    print(f"xw_dense {case.name} {case.dt} {case.n}x{case.M}x{case.P}: {f.kind}<{f.a},{f.b}> blocks {f.blocks} max_trips {f.max_trips}: "
          f"max err / bound = {ratio:.3f}")
    assert ratio <= 1.0

    # bits: the tile kernel under every gate, and every arm an override leads to
    tile = _tile_reference(case, Xv, Wv)
    assert _same(got, tile), "against the tile kernel on chunks of 4096 rows"
    for ov in D.OVERRIDES:
        if ov in env:
            continue
        with _lib.tuning(**env, **{ov: "1"}):
            other, _, f2 = _run(case, Xv, Wv, want_form=True)
        assert _same(other, got), (ov, f2)
    del tile

    # activation: NaN and -0 go to +0 (K.cpp:2586-2590, relu_f16)
    assert _same(act, torch.where(got > 0, got, torch.zeros_like(got)))

    # pad columns
    assert not _bits(full[:, case.P:]).any() and not _bits(act_full[:, case.P:]).any()


def test_xw_dense_no_rows_launches_nothing():
    from sgracex1_amd import ops
    for dt in (torch.float16, torch.float32):
        X = torch.empty((0, 40), dtype=dt, device="cuda")
        Wt = torch.ones((24, 40), dtype=dt, device="cuda")
        buf = torch.full((4 * 32,), -7.5, dtype=dt, device="cuda")
        out = torch.as_strided(buf, (0, 24), (32, 1), 32)
        f = ops.xw_dense_form(X, Wt, out=out)
        assert f.kind == "none" and f.waves == 0 and f.max_trips == 0
        assert ops.xw_dense(X, Wt, out=out).shape == (0, 24)
        assert torch.equal(buf, torch.full_like(buf, -7.5))
        assert ops.xw_dense(X, Wt).shape == (0, 24)


@pytest.mark.parametrize("name", D.PER_KIND)
def test_xw_dense_masks(name):
    """X and Wt as views into larger buffers (ldx = M + 2, even; ldw = M + 4; three rows before, five after; X at an address
    that is 4 mod 16) whose pad columns and outside rows hold NaN in one run and 1e30 in another: the k-tails (load_k8 /
    load_k4, the ring's tail_mask, the fill masks of the copies of W^T in LDS) keep out what lies beyond M -- the same arm,
    the same bits as the contiguous run."""
    case = D.BY_NAME[name]
    assert not case.x and not case.w and not case.env
    X, Wt = _operands(case.n, case.M, case.P, case.dt)
    got, _, f = _run(case, X, Wt, want_form=True)
    assert (f.kind, f.a, f.b) == case.arm
    es = X.element_size()
    for fill in (NAN, 1e30):
        Xv = _view(X, case.M + 2, skip=4 // es, fill=fill, before=3, after=5)
        Wv = _view(Wt, case.M + 4, fill=fill, before=3, after=5)
        assert Xv.data_ptr() % 16 == (4 + 3 * (case.M + 2) * es) % 16 and Xv.stride(0) % 2 == 0      # (the buffer: 4 mod 16)
        other, _, f2 = _run(case, Xv, Wv, want_form=True)
        assert f2[:3] == f[:3], f2
        assert _same(other, got), f"views into buffers of {fill}"
    # the values the run is compared with are right: inside the bound
    want, bound = _bound(X, Wt, case.dt)
    assert ((got.double() - want).abs() <= bound).all()


SENTINEL = -12345.5


def _vec_rule(dt, kind, b, ptr, ldh):
    """include/sgx.h: H leaves in vector stores unless H or its pitch is under-aligned -- 8 bytes (fp16) or 16 (fp32), and
    16 bytes with a pitch of whole 16-byte pieces for the fp16 forms that store 8 columns at once"""
    if dt == "f32":
        return ptr % 16 == 0 and ldh % 4 == 0
    if kind == "wlds" or (kind == "stationary" and b % 2 == 0):
        return ptr % 16 == 0 and ldh % 8 == 0
    return ptr % 8 == 0 and ldh % 4 == 0


@pytest.mark.parametrize("name", D.PER_KIND)
def test_xw_dense_guard_bands(name):
    """out= as a view of a sentinel-filled buffer, two rows before and three after: 16-byte aligned at a pitch that is a
    multiple of 8; a pitch that is no multiple of 8 (and none of 4); a base off by 8 bytes; ldh = P ragged (P - 3 columns).
    The result is the contiguous run's bit for bit, every element outside [n_rows][ldh] keeps the sentinel, and the form's
    vector-stores flag is what the alignment rule says, either way."""
    from sgracex1_amd import ops
    case = D.BY_NAME[name]
    X, Wt = _operands(case.n, case.M, case.P, case.dt)
    n, P, es = case.n, case.P, X.element_size()
    ld0 = D.layout(case)[4]
    flags = set()
    for what, W, ldh, skip in (("aligned", Wt, ld0 + 8, 0), ("pitch % 8 != 0", Wt, ld0 + 3, 0), ("base + 8 bytes", Wt, ld0 + 8, 8 // es),
                               ("ldh = P ragged", Wt[:P - 3], P - 3, 0)):
        p = W.shape[0]
        buf, out = _out(case, n, p, ldh, skip, fill=SENTINEL, before=2, after=3)
        f = ops.xw_dense_form(X, W, out=out)
        assert f.vec == _vec_rule(case.dt, f.kind, f.b, out.data_ptr(), ldh), (what, f)
        flags.add(f.vec)
        got = ops.xw_dense(X, W, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert _same(got, ops.xw_dense(X, W)), what
        lo, hi = skip + 2 * ldh, skip + (2 + n) * ldh
        assert (buf[:lo] == SENTINEL).all() and (buf[hi:] == SENTINEL).all(), what
        assert not _bits(buf[lo:hi].view(n, ldh)[:, p:]).any(), what
    assert flags == {True, False}


@pytest.mark.parametrize("name", D.PER_KIND)
def test_xw_dense_hostile_values(name):
    """Whole rows of X NaN (rows 0, 15, 16, the last row of a 128-row tile, n - 1), +inf in the first and -inf in the last k
    of two other rows, one row of Wt NaN: float64's non-finite pattern element by element, the finite elements within the
    bound; and the activation on these values -- NaN, -inf and -0 go to +0, +inf stays (K.cpp:2586-2590, relu_f16)."""
    case = D.BY_NAME[name]
    X, Wt = (t.clone() for t in _operands(case.n, case.M, case.P, case.dt))
    n = case.n
    X[torch.tensor([0, 15, 16, 127, n - 1], device="cuda")] = NAN
    X[5, 0], X[40, case.M - 1] = float("inf"), float("-inf")
    Wt[3] = NAN
    got, _, f = _run(case, X, Wt, want_form=True)
    assert (f.kind, f.a, f.b) == case.arm
    want, bound = _bound(X, Wt, case.dt)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got == float("inf"), want == float("inf")) and torch.equal(got == float("-inf"), want == float("-inf"))
    fin = torch.isfinite(want)
    assert fin[1, 0] and not fin[:, 3].any() and not fin[0].any() and fin.sum() == (n - 7) * (case.P - 1)
    assert torch.where(fin, (got.double() - want).abs() <= bound, torch.ones_like(fin)).all()
    act = _run(case, X, Wt, relu=True)[0]
    assert _same(act, torch.where(got > 0, got, torch.zeros_like(got)))
    assert torch.isnan(got).any() and (got == float("-inf")).any() and (act == float("inf")).any()
    assert not torch.isnan(act).any() and not _bits(act[0]).any() and not _bits(act[:, 3]).any()          # NaN -> +0, bit for bit
