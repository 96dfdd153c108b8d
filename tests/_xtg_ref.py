"""Plain-Python restatement of the host side of sgx_xt_g (sgracex1_amd/csrc/xtg.hip): geometry() -- the slabs of graph rows,
the padded tile sizes and the arrangement of a workgroup's 8 sub-tiles -- and the entry point's rule for which kernel a call
runs.  The shape table the tests share stands here too, with the arm each row is meant to reach, so that the CPU test
can say which template instantiations the GPU tests execute.

Arms:
  "wg"      xtg_partial_wg_kernel<TX, WM, WP>: n_rows >= 16384, WM x WP from geometry()
  "vec"     xtg_partial_vec_kernel<TX>: wavefront tiles, 16-byte loads through buffer resources
  "scalar"  xtg_partial_kernel<TX>: one element per load; unaligned rows, tables over 4 GiB, or SGX_XTG_SCALAR
  "zero"    n_rows == 0: the output is cleared, no kernel runs
"""
import torch

TILE = 64                  # kTile
WG_MIN_ROWS = 16384        # sgx_xt_g: "enough rows to fill the device with workgroup tiles"
OFFSET_LIMIT = 0xFFF00000  # the tables must fit 32-bit byte offsets


def align256(nbytes):
    return (nbytes + 255) // 256 * 256


def geometry(n_rows, M, P):
    """(n_slabs, rows_per_slab, m_pad, p_pad, wm) as geometry() in xtg.hip computes them."""
    m_pad = (M + TILE - 1) // TILE * TILE
    p_pad = (P + TILE - 1) // TILE * TILE
    mt, pt = m_pad // TILE, p_pad // TILE
    best, best_wm = 1 << 40, 8
    for wm in (8, 4, 2, 1):                                   # strict "<": a tie stays with the larger wm
        wp = 8 // wm
        tiles = ((mt + wm - 1) // wm) * ((pt + wp - 1) // wp)
        if tiles < best:
            best, best_wm = tiles, wm
    tile_bytes = m_pad * p_pad * 4
    slabs = 512 // best                                       # one round of workgroups on 256 CUs
    slabs = min(slabs, (n_rows + 63) // 64)                   # >= 64 graph rows per slab
    slabs = min(slabs, (64 << 20) // tile_bytes)              # partials capped at 64 MiB
    slabs = max(slabs, 1)
    rps = (n_rows + slabs - 1) // slabs
    rps = max((rps + 15) // 16 * 16, 16)                      # (16 where n_rows == 0)
    n_slabs = max((n_rows + rps - 1) // rps, 1)
    return n_slabs, rps, m_pad, p_pad, best_wm


def workspace_bytes(n_rows, M, P):
    """sgx_xt_g_workspace_bytes."""
    if n_rows < 0 or M < 1 or P < 1:
        return 0
    n_slabs, _, m_pad, p_pad, _ = geometry(n_rows, M, P)
    return align256(n_slabs * m_pad * p_pad * 4)


def arm(n_rows, dtype, ldx, ldg, x_addr=0, g_addr=0, scalar_override=False, wave_tiles_override=False):
    """Which partial-product kernel sgx_xt_g launches.  x_addr / g_addr: the operands' addresses (only their value
    mod 4 matters); the overrides are SGX_XTG_SCALAR and SGX_XTG_WAVE_TILES."""
    if n_rows == 0:
        return "zero"
    es = 2 if dtype == torch.float16 else 4
    vec = (not scalar_override and x_addr % 4 == 0 and (ldx * es) % 4 == 0 and g_addr % 4 == 0
           and n_rows * ldx * es < OFFSET_LIMIT and n_rows * ldg * 4 < OFFSET_LIMIT)
    if vec and n_rows >= WG_MIN_ROWS and not wave_tiles_override:
        return "wg"
    return "vec" if vec else "scalar"


def padded_ld(width):
    """A row pitch over `width` that keeps fp16 rows dword-aligned: the next even number above it (602 -> 604, 7 -> 8)."""
    return width + 2 - (width & 1)


def arrangement(n_rows, M, P):
    """"WMxWP" of the workgroup kernel for this shape."""
    wm = geometry(n_rows, M, P)[4]
    return f"{wm}x{8 // wm}"


N0 = WG_MIN_ROWS
# (n_rows, M, P, the arm operands with dword-aligned rows reach -- contiguous ones unless X is fp16 of an odd width, and
# the padded views of the mask test always --, the arrangement geometry() picks, why the row is here)
SHAPES = [
    (N0, 64, 64, "wg", "8x1", "every arrangement has one tile: the tie goes to the larger WM; 7 of 8 sub-tiles cut by mt < m_pad"),
    (N0, 300, 7, "wg", "8x1", "ragged M and P, m_pad = 320 < 512"),
    (N0, 602, 128, "wg", "4x2", "the Reddit shape; 602 is no multiple of 4"),
    (N0, 64, 256, "wg", "2x4", "tie between 2x4 and 1x8"),
    (N0, 128, 256, "wg", "2x4", "both sub-tile rows of the 2x4 tile in use"),
    (N0, 64, 512, "wg", "1x8", "XCH = 256 < 512 threads"),
    (N0, 7, 300, "wg", "1x8", "ragged M and P, p_pad = 320 < 512"),
    (N0, 65, 2, "wg", "8x1", "the [n, 2] G of the GAT attention gradient"),
    (N0, 33, 1, "wg", "8x1", "one column of G"),
    # other row counts, one table row each
    (N0 + 1, 64, 256, "wg", "2x4", "the last slab holds one row"),
    (N0 - 1, 602, 128, "vec", "4x2", "just below the workgroup kernel's threshold"),
    (N0 + 37, 7, 300, "wg", "1x8", "the last slab ends inside a 16-row step"),
    (1, 65, 2, "vec", "8x1", "one row"),
    (3, 7, 300, "vec", "1x8", "less than one quad of rows"),
    (63, 64, 64, "vec", "8x1", "one slab, short of 64 rows"),
    (64, 300, 7, "vec", "8x1", "one slab of exactly 64 rows"),
    (65, 64, 512, "vec", "1x8", "two slabs, 48 rows and 17"),
    (1000, 602, 128, "vec", "4x2", "16 slabs of 64 rows, the last ragged"),
    (0, 64, 64, "zero", "8x1", "no rows: zeros"),
]
DTYPES = (torch.float16, torch.float32)

# geometry() for every row above, worked out by hand from the rules in xtg.hip (tests/test_xtg_ref_cpu.py pins the
# restatement to these, and the library's workspace size to the restatement)
GEOMETRY = {
    (N0, 64, 64): (256, 64, 64, 64, 8),            # 1 tile: 512 slabs wanted, 16384 / 64 = 256 allowed
    (N0, 300, 7): (256, 64, 320, 64, 8),
    (N0, 602, 128): (147, 112, 640, 128, 4),       # 3 tiles: 170 slabs wanted, ceil(16384 / 170) = 97 -> 112 rows, 147 slabs
    (N0, 64, 256): (256, 64, 64, 256, 2),
    (N0, 128, 256): (256, 64, 128, 256, 2),
    (N0, 64, 512): (256, 64, 64, 512, 1),
    (N0, 7, 300): (256, 64, 64, 320, 1),
    (N0, 65, 2): (256, 64, 128, 64, 8),
    (N0, 33, 1): (256, 64, 64, 64, 8),
    (N0 + 1, 64, 256): (257, 64, 64, 256, 2),      # 257 slabs allowed, ceil(16385 / 257) = 64 rows: slab 256 is row 16384 alone
    (N0 - 1, 602, 128): (147, 112, 640, 128, 4),
    (N0 + 37, 7, 300): (257, 64, 64, 320, 1),      # slab 256 holds 37 rows: two steps of 16 and one of 5
    (1, 65, 2): (1, 16, 128, 64, 8),
    (3, 7, 300): (1, 16, 64, 320, 1),
    (63, 64, 64): (1, 64, 64, 64, 8),
    (64, 300, 7): (1, 64, 320, 64, 8),
    (65, 64, 512): (2, 48, 64, 512, 1),            # ceil(65 / 2) = 33 -> 48 rows, then 17
    (1000, 602, 128): (16, 64, 640, 128, 4),
    (0, 64, 64): (1, 16, 64, 64, 8),               # no rows: one slab (of the smallest size) that nothing fills
}
