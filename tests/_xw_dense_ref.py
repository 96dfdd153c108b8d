"""Dense X.W (csrc/xw_dense.hip, csrc/xw_dense_wlds.hip): the deterministic inputs its arm tests run on, the float64
restatement with the house bound of _spmm_acc_ref, and the table of cases, one per arm of sgx_xw_dense -- shared by
tests/test_xw_dense_ref_cpu.py (no GPU: the arms the table reaches, the bound's lack of slack) and
tests/test_gpu_xw_dense_arms.py.  Plain numpy; nothing here touches the GPU.

Inputs: |x| and |w| in [1/4, 1] with a random sign and a full random mantissa, rounded to the storage type -- every term
of a sum is at least 1/16 in magnitude, on the last k of every row as on every other, so one term lost or gained moves a
sum by 2^-4 against a bound of (M + 2) 2^-24 (|X| |W|) + one store rounding (about 1.5e-2 at fp16 and M = 602).

Bound, elementwise, with scale = |X|64 . |W|64: an fp32 sum of M products in ANY order lies within (M + 2) 2^-24 scale of
the float64 sum (each of the M - 1 additions and the rounding of what enters them at most 2^-24 of the partial sums, which
scale bounds; products of fp16 or fp32 operands are exact in float64, and the fp32 kernels' fused multiply-adds round once
per term); the stored result adds 2^-11 |want| + 2^-25 (fp16: half an ulp, and half the smallest subnormal) or 2^-24 |want|.
"""
import collections

import numpy as np

import _spmm_acc_ref as R

U = R.U                                       # 2^-24: the unit of the sum's bound
OVERRIDES = ("SGX_XW_NO_WLDS", "SGX_XW_NO_STATIONARY_F32", "SGX_XW_NO_LDS", "SGX_XW_SHORT_TILES")
CHUNK = 4096                                  # rows per call of the tile kernel's reference run: under every gate (8192, 32768)


def signed(rng, shape):
    """float32 values of magnitude in [1/4, 1] with a random sign"""
    mag = np.float32(0.25) + np.float32(0.75) * rng.random(shape, dtype=np.float32)
    return mag * (rng.integers(0, 2, shape, dtype=np.int8) * 2 - 1).astype(np.float32)


def operands(n, M, P, dt, seed=0):
    """(X [n, M], Wt [P, M]) in the storage type"""
    rng = np.random.default_rng(1000003 * (n % 100003) + 1009 * M + P + 7919 * seed)
    return signed(rng, (n, M)).astype(R.NP_DTYPE[dt]), signed(rng, (P, M)).astype(R.NP_DTYPE[dt])


def bound(M, scale, want, dt, unit=U):
    """the elementwise bound from scale = |X| . |W| and the float64 product, as numpy arrays or torch tensors alike: the ONE
    expression tests/test_xw_dense_ref_cpu.py shows to have no slack and tests/test_gpu_xw_dense_arms.py holds the kernels to"""
    store = (2.0 ** -11 * abs(want) + 2.0 ** -25) if dt == "f16" else 2.0 ** -24 * abs(want)
    return (M + 2.0) * unit * scale + store


def reference(X, Wt, dt, unit=U):
    """(want, bound) of the stored X . Wt^T in float64"""
    X64, W64 = np.asarray(X, np.float64), np.asarray(Wt, np.float64)
    want = X64 @ W64.T
    return want, bound(X.shape[1], np.abs(X64) @ np.abs(W64).T, want, dt, unit)


def k_step(dt):
    """k elements one MFMA step of the kernels consumes"""
    return 32 if dt == "f16" else 16


# ---- the cases ----------------------------------------------------------------------------------------------------------
# x / w / h: how the operand is laid out -- None: contiguous in a fresh allocation (H: at the library's own pitch, or at
# `ldh`); otherwise (pitch in elements, elements the view's address lies past a 256-byte aligned one).
# arm: (kind, a, b) as ops.xw_dense_form names it; blocks: column blocks or groups; trips: max_trips at least this;
# wgs: workgroups per CU (None: not asserted).
Case = collections.namedtuple("Case", "name dt n M P ldh env x w h arm blocks trips wgs why")


def _c(name, dt, n, M, P, arm, blocks, why, ldh=None, env=(), x=None, w=None, h=None, trips=1, wgs=None):
    return Case(name, dt, n, M, P, ldh, tuple(env), x, w, h, arm, blocks, trips, wgs, why)


BIG = 32768 + 37
CASES = [
    # fp16 tile kernel (under 8192 rows)
    _c("h_tile_1x4", "f16", 1, 7, 10, ("tile", 1, 4), 1, "one row, K = 7: the scalar k-tail only"),
    _c("h_tile_2x4", "f16", 17, 40, 30, ("tile", 2, 4), 1, "K = 40: a k-tail of exactly 8, a second row tile of one row"),
    _c("h_tile_4x4", "f16", 1037, 130, 64, ("tile", 4, 4), 1, "K = 130: a tail of 2 in the fifth step; several workgroups"),
    _c("h_tile_8x2", "f16", 1037, 602, 128, ("tile", 8, 2), 1, "K = 602: rows aligned to 4 bytes only, 19 steps"),
    _c("h_tile_16x1", "f16", 1037, 40, 256, ("tile", 16, 1), 1, "a whole block of 256 columns"),
    _c("h_tile_two_blocks", "f16", 1037, 130, 300, ("tile", 4, 4), 2, "P = 300 at a pitch of 320: <16,1> then <4,4> with pad columns"),
    _c("h_tile_7", "f16", 1037, 7, 64, ("tile", 4, 4), 1, "K = 7 on many rows"),
    _c("h_tile_under_gate", "f16", 8191, 40, 64, ("tile", 4, 4), 1, "8191 rows: the last shape under the stationary gate"),
    # fp16 tall tiles
    _c("h_tall_8x4", "f16", BIG, 130, 128, ("tile", 8, 4), 1, "tall tile, reachable with SGX_XW_NO_LDS only", env=["SGX_XW_NO_LDS"]),
    _c("h_tall_16x2", "f16", BIG, 130, 256, ("tile", 16, 2), 1, "tall tile, reachable with SGX_XW_NO_LDS only", env=["SGX_XW_NO_LDS"]),
    # fp16 stationary
    _c("h_st_2x8_gate", "f16", 8192, 40, 128, ("stationary", 2, 8), 1, "8192 rows exactly: the gate", wgs=8),
    _c("h_st_2x4", "f16", 8229, 64, 64, ("stationary", 2, 4), 1, "K = 64: two whole k-steps"),
    _c("h_st_2x2", "f16", 8229, 7, 30, ("stationary", 2, 2), 1, "K = 7: the second k-step all zeros"),
    _c("h_st_2x1", "f16", 8229, 40, 10, ("stationary", 2, 1), 1, "one column tile: the unpaired 8-byte stores"),
    _c("h_st_4x4", "f16", 8229, 100, 64, ("stationary", 4, 4), 1, "K = 100: a tail of 4 in the fourth step"),
    _c("h_st_4x2", "f16", 8229, 128, 30, ("stationary", 4, 2), 1, "K = 128: four whole steps"),
    _c("h_st_4x1", "f16", 8229, 65, 10, ("stationary", 4, 1), 1, "K = 65: one element in the third step"),
    _c("h_st_past_ldh", "f16", 8229, 40, 200, ("stationary", 2, 8), 2, "ldh = 208: the second group of 128 columns reaches past ldh", ldh=208),
    _c("h_st_trips", "f16", 108101, 100, 300, ("stationary", 4, 4), 5,
       "five column groups: 8195 wavefronts wanted, 8196 in 2049 workgroups, one idle; 1639 streams walk 3379 row tiles -- three trips, the "
       "last ragged (five groups need P > 256: the one shape with many rows that is wider than 64)", trips=3),
    # fp16 128 x 128 tiles through LDS, reached without an override
    _c("h_lds_odd_ldx", "f16", BIG, 130, 64, ("tile_lds", 8, 8), 1, "an odd pitch of X keeps the buffer loads of the ring away", x=(131, 0)),
    _c("h_lds_x_2mod4", "f16", BIG, 130, 64, ("tile_lds", 8, 8), 1, "X at an address that is 2 mod 4", x=(132, 1)),
    _c("h_lds_3_blocks", "f16", BIG, 602, 300, ("tile_lds", 8, 8), 3, "three column blocks of 128: one more than W^T in LDS takes"),
    _c("h_lds_out_8", "f16", BIG, 130, 64, ("tile_lds", 8, 8), 1, "out= 8 bytes off a 16-byte boundary", h=(64, 4)),
    # fp16 W^T in LDS, X through the ring
    _c("h_wlds_2", "f16", 32768, 130, 30, ("wlds", 2, 1), 1, "32768 rows exactly; K = 130: KS2 = 3, the least the store schedule allows", wgs=2),
    _c("h_wlds_4", "f16", BIG, 162, 64, ("wlds", 4, 1), 1, "KS = 6 (even), M % 32 = 2", wgs=2),
    _c("h_wlds_8", "f16", BIG, 160, 128, ("wlds", 8, 1), 1, "KS = 5 (odd), M % 32 = 0: no tail to mask", wgs=2),
    _c("h_wlds_8_602", "f16", BIG, 602, 128, ("wlds", 8, 1), 1, "K = 602: KS = 19 (odd), M % 32 = 26; 154 KB of W^T, one workgroup per CU", wgs=1),
    _c("h_wlds_8_2", "f16", BIG, 130, 256, ("wlds", 8, 2), 2, "two column blocks of 128", wgs=2),
    _c("h_wlds_4_2", "f16", BIG, 650, 128, ("wlds", 4, 2), 2, "K = 650: W^T of 128 columns does not fit (KS = 21); two blocks of 64", wgs=1),
    _c("h_wlds_trips", "f16", 8 * 32768 + 4165, 130, 64, ("wlds", 4, 1), 1, "4096 wavefronts walk 8323 row tiles: three trips, the last ragged",
       trips=3, wgs=2),
    # fp32 tile kernel
    _c("f_tile_1x4", "f32", 17, 7, 3, ("tile", 1, 4), 1, "K = 7: a scalar tail of 3 in the second lane quad"),
    _c("f_tile_2x4", "f32", 1, 40, 30, ("tile", 2, 4), 1, "one row; K = 40: a tail of 8 in the third step"),
    _c("f_tile_4x4", "f32", 1037, 130, 64, ("tile", 4, 4), 1, "K = 130: a tail of 2 in the ninth step"),
    _c("f_tile_8x2", "f32", 1037, 602, 128, ("tile", 8, 2), 1, "K = 602: rows aligned to 8 bytes only"),
    _c("f_tile_two_blocks", "f32", 1037, 40, 300, ("tile", 4, 4), 2, "P = 300 at a pitch of 320: <16,1> then <4,4>"),
    _c("f_tile_256", "f32", 1037, 7, 256, ("tile", 16, 1), 1, "a whole block of 256 columns"),
    _c("f_tall_8x4", "f32", BIG, 130, 128, ("tile", 8, 4), 1, "K > 128 on 32 K rows: the tall tile"),
    _c("f_tall_16x2", "f32", BIG, 130, 256, ("tile", 16, 2), 1, "K > 128 on 32 K rows: the tall tile"),
    # fp32 stationary
    *[_c(f"f_st_{kb}x{ntw}", "f32", 8229, M, P, ("stationary", kb, ntw), 1, f"K = {M}", wgs=2)
      for kb, M in ((2, 7), (4, 40), (8, 100)) for ntw, P in ((4, 64), (2, 30), (1, 3))],
    _c("f_st_trips", "f32", BIG, 40, 3, ("stationary", 4, 1), 1, "2048 wavefronts walk 2051 row tiles: a second, ragged trip", trips=2),
    _c("f_st_ldw", "f32", BIG, 100, 128, ("stationary", 8, 4), 2, "ldw = 102, no multiple of 4: a wide output kept off the LDS form; three trips", w=(102, 0), trips=3),
    # fp32 W^T in LDS
    _c("f_wlds_4x8", "f32", BIG, 40, 128, ("wlds", 4, 8), 1, "K = 40: a tail of 8 in the third k block"),
    _c("f_wlds_4x16", "f32", BIG, 64, 256, ("wlds", 4, 16), 1, "K = 64: four whole k blocks"),
    _c("f_wlds_8x8", "f32", BIG, 100, 100, ("wlds", 8, 8), 1, "P = 100 at a pitch of 128: 28 pad columns"),
    _c("f_wlds_8x16", "f32", BIG, 128, 256, ("wlds", 8, 16), 1, "K = 128, P = 256: the table fills the LDS"),
    _c("f_wlds_2_blocks", "f32", BIG, 68, 300, ("wlds", 8, 8), 2, "P = 300 at a pitch of 320: blocks of 256 and 64"),
    _c("f_wlds_3_blocks", "f32", BIG, 36, 602, ("wlds", 4, 8), 3, "P = 602 at a pitch of 608: blocks of 256, 256, 96"),
    _c("f_wlds_pad_block", "f32", BIG, 100, 250, ("wlds", 8, 8), 2, "ldh = 272: the second block holds pad columns only", ldh=272),
    _c("f_wlds_trips", "f32", 2 * 32768 + 37, 40, 128, ("wlds", 4, 8), 1, "2048 wavefronts walk 4099 row tiles: three trips, the last ragged",
       trips=3),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the arms section 3 of the work asks for, as (dtype, kind, a, b): what the table must reach, exactly
ARMS = {("f16", "tile", nt, mt) for nt, mt in ((1, 4), (2, 4), (4, 4), (8, 2), (16, 1), (8, 4), (16, 2))} | \
       {("f16", "stationary", ks, ntw) for ks, ntw in ((2, 8), (2, 4), (2, 2), (2, 1), (4, 4), (4, 2), (4, 1))} | \
       {("f16", "tile_lds", 8, 8)} | \
       {("f16", "wlds", nt, n_cb) for nt, n_cb in ((2, 1), (4, 1), (8, 1), (8, 2), (4, 2))} | \
       {("f32", "tile", nt, mt) for nt, mt in ((1, 4), (2, 4), (4, 4), (8, 2), (16, 1), (8, 4), (16, 2))} | \
       {("f32", "stationary", kb, ntw) for kb in (2, 4, 8) for ntw in (4, 2, 1)} | \
       {("f32", "wlds", kb, nt) for kb in (4, 8) for nt in (8, 16)}

# one case per kind and dtype for the masks, the guard bands and the hostile values
PER_KIND = ["h_tile_4x4", "h_st_4x4", "h_lds_out_8", "h_wlds_4", "f_tile_4x4", "f_st_8x4", "f_wlds_8x8"]
assert {(BY_NAME[c].dt, BY_NAME[c].arm[0]) for c in PER_KIND} == {(dt, kind) for dt, kind, _, _ in ARMS}


def pitch(P, dt):
    """the library's own pitch of H (sgx_ldh / ops.table_pitch), restated"""
    es = 2 if dt == "f16" else 4
    row = (P * es + 15) // 16 * 16
    if row < 128:
        p = 16
        while p < row:
            p *= 2
    else:
        lines = (row + 127) // 128 * 128
        p = lines if 3 * lines <= 4 * row else row
    return p // es


def layout(case):
    """(ldx, x_skip, ldw, w_skip, ldh, h_skip) in elements of a case"""
    ldx, xs = case.x or (case.M, 0)
    ldw, ws = case.w or (case.M, 0)
    ldh, hs = case.h or (case.ldh or pitch(case.P, case.dt), 0)
    return ldx, xs, ldw, ws, ldh, hs


def max_trips(case, waves, blocks):
    """the most row tiles one wavefront of a persistent grid walks (ops.unpack_xw_dense_form, restated)"""
    tiles = -(-case.n // (32 if case.dt == "f16" else 16))
    if case.arm[0] == "stationary":
        return -(-tiles // (waves // blocks))
    if case.arm[0] == "wlds":
        return -(-tiles // waves)
    return 1
