"""Synthetic graphs that put an exact number of items through each of the sampler's exclusive scans (scan_launch in
csrc/sample_device.h), for tests/test_gpu_sampler_scan.py; numpy, seeded, no GPU.  tests/test_sampler_cpu.py holds every
builder to the counts it claims and to the seam property below.

The scan works in tiles of TILE items, and one workgroup scans up to 1024 tile sums per round, so TOP items are the most
one round covers.  A seam tile is one in which the scan changes path: the first, the last (ragged) one, and the tile on
each side of every round boundary below the item count.  In every seam tile the items' values are of both kinds -- zero
and non-zero -- so that a sum carried wrongly into or out of the tile moves an output; a seam tile of a single item
(counts of the form k * TILE + 1) holds a non-zero one, its neighbour tile both kinds.

A hop's columns are built slot by slot from four kinds: FRESH (a node no seed and no earlier slot names: the only slots
whose first-appearance flag is 1, each on a node of its own), SEED (some seed), SELF (the seed whose row the slot is
in: a self loop) and REPEAT (the node of an earlier FRESH slot).  Degrees stay at 3 or below."""
import functools
from types import SimpleNamespace

import numpy as np

TILE = 2048
TOP = TILE * 1024
SIZES = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, TOP - 1, TOP, TOP + 1, 2 * TOP + 1]

FRESH, SEED, SELF, REPEAT = 0, 1, 2, 3


def seam_tiles(n):
    """The item ranges [a, b) of the seam tiles of a scan over n items."""
    if n < 1:
        return []
    tiles = {0, (n - 1) // TILE}
    for r in range(1, (n - 1) // TOP + 1):
        tiles |= {r * TOP // TILE - 1, r * TOP // TILE}
    return [(t * TILE, min((t + 1) * TILE, n)) for t in sorted(tiles)]


def seams_hold(nonzero):
    """The seam property of a scan whose items' values are non-zero where `nonzero` (bool [n]) says so."""
    nonzero = np.asarray(nonzero, bool)
    return all(nonzero[a] if b - a == 1 else nonzero[a:b].any() and not nonzero[a:b].all() for a, b in seam_tiles(len(nonzero)))


def _row_degrees(rng, rows, choices):
    """Degrees of `rows` frontier rows drawn from `choices`; every seam tile opens on an empty row and closes on a full one."""
    deg = rng.choice(np.asarray(choices, np.int64), rows)
    for a, b in seam_tiles(rows):
        if b - a > 1:
            deg[a] = 0
        deg[b - 1] = max(choices)
    return deg


def _degrees_with_sum(rng, total):
    """Degrees from {0, 1, 2, 3} that add up to exactly `total`: drawn until the running sum gets there, the last one cut."""
    deg = np.concatenate([rng.integers(0, 4, total), np.ones(total, np.int64)])        # (the ones: the sum does get there)
    run = np.cumsum(deg)
    last = int(np.searchsorted(run, total))
    deg = deg[:last + 1]
    deg[last] -= run[last] - total
    return deg


def _slot_kinds(rng, slots):
    """A kind per slot, 2 in 5 FRESH; every seam tile opens SEED, FRESH, REPEAT and closes FRESH."""
    kinds = rng.choice(np.asarray([FRESH, FRESH, SEED, SELF, REPEAT]), slots)
    for a, b in seam_tiles(slots):
        for i, k in enumerate((SEED, FRESH, REPEAT)):
            if a + i < b - 1:
                kinds[a + i] = k
        kinds[b - 1] = FRESH
    return kinds


def _hop_graph(rng, deg, kinds, deg_new=None, spare=None):
    """The graph of one planned hop: len(deg) seeds with these degrees whose sum(deg) slots, in frontier order, are of
    these kinds.  deg_new: the degrees of the FRESH nodes' own rows, in order of appearance (their columns are uniform over
    all nodes); None: empty rows.  A few nodes more (`spare`) are in the graph and never named by a seed's row.
    -> rowptr, col, seeds (int64), frontier / edges / new: the rows, sampled edges and new nodes of hop 0 by construction,
    fresh_ids: those new nodes in order of appearance."""
    B, slots = len(deg), int(deg.sum())
    assert len(kinds) == slots and (deg >= 0).all() and (deg <= 3).all()
    fresh = kinds == FRESH
    n_fresh = int(fresh.sum())
    n = B + n_fresh + (max(8, n_fresh // 8) if spare is None else spare)
    ids = rng.permutation(n)                                # seeds and new nodes are a real gather, not a range
    seeds, fresh_ids = ids[:B], ids[B:B + n_fresh]
    slot_col = seeds[rng.integers(0, B, slots)]             # SEED
    own = seeds[np.repeat(np.arange(B), deg)]
    slot_col[kinds == SELF] = own[kinds == SELF]
    slot_col[fresh] = fresh_ids
    before = np.cumsum(fresh) - fresh                       # FRESH slots ahead of each slot
    rep = (kinds == REPEAT) & (before > 0)                  # (a REPEAT with nothing to repeat stays a SEED)
    slot_col[rep] = fresh_ids[(rng.random(slots) * before).astype(np.int64)[rep]]
    node_deg = np.zeros(n, np.int64)
    node_deg[seeds] = deg
    if deg_new is not None:
        node_deg[fresh_ids] = deg_new
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(node_deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1]))
    ends = np.cumsum(deg)
    col[np.repeat(rowptr[seeds] - (ends - deg), deg) + np.arange(slots)] = slot_col
    return SimpleNamespace(rowptr=rowptr, col=col, seeds=seeds, frontier=B, edges=slots, new=n_fresh, fresh_ids=fresh_ids)


@functools.lru_cache(maxsize=None)
def frontier_graph(rows, choices=(0, 1, 2, 3)):
    """A batch of exactly `rows` seeds: the RowCounts scan of hop 0 runs over `rows` items."""
    rng = np.random.default_rng([1, rows, len(choices)])
    deg = _row_degrees(rng, rows, choices)
    return _hop_graph(rng, deg, _slot_kinds(rng, int(deg.sum())))


@functools.lru_cache(maxsize=None)
def edge_graph(slots):
    """A batch whose rows hold exactly `slots` edges: the FirstSeen scan of hop 0 runs over `slots` items."""
    rng = np.random.default_rng([2, slots])
    return _hop_graph(rng, _degrees_with_sum(rng, slots), _slot_kinds(rng, slots))


@functools.lru_cache(maxsize=None)
def second_hop_graph(new):
    """A batch whose hop 0 finds exactly `new` nodes, with rows of their own: the RowCounts scan of hop 1 runs over `new`
    items behind a frontier and an edge count that are not 0."""
    rng = np.random.default_rng([3, new])
    kinds = rng.choice(np.asarray([FRESH] * 4 + [SEED, SELF, REPEAT]), 2 * new)
    kinds = np.concatenate([kinds, np.full(new, FRESH)])   # (the tail: `new` FRESH slots do occur)
    slots = int(np.searchsorted(np.cumsum(kinds == FRESH), new)) + 1
    kinds = kinds[:slots]
    return _hop_graph(rng, _degrees_with_sum(rng, slots), kinds, deg_new=_row_degrees(rng, new, (0, 1, 2, 3)))


@functools.lru_cache(maxsize=None)
def node_batch_graph(nodes, new=777):
    """A batch whose one hop with every neighbour samples exactly `nodes` nodes, the last `new` of them (fewer than a tile)
    found by the hop: the LoopMissing and the FeatureRows scan run over `nodes` items.  Every seam tile of the sampled rows
    opens on a row without a self loop and holds one with; the rows the hop found are empty, so without.  x: a dense
    [n_nodes, 3] fp32 feature matrix whose rows store 0 to 3 entries, every seam tile of n_id opening on an empty row and
    closing on a full one.  -> the graph of _hop_graph with x and n_id (by construction)."""
    rng = np.random.default_rng([4, nodes])
    new = min(new, nodes // 2)
    B = nodes - new
    deg = rng.integers(0, 4, B)
    loops = []                                              # rows that open on a self loop
    for a, b in seam_tiles(nodes):
        if a < B:
            deg[a] = 0
        if a + 1 < B:
            deg[a + 1] = 3
            loops.append(a + 1)
    slots = int(deg.sum())
    assert slots - len(loops) >= new
    kinds = rng.choice(np.asarray([SEED, SELF, REPEAT]), slots)
    starts = np.cumsum(deg) - deg
    fixed = starts[np.asarray(loops, np.int64)]
    kinds[fixed] = SELF
    free = np.setdiff1d(np.arange(slots), fixed)
    kinds[rng.permutation(free)[:new]] = FRESH
    g = _hop_graph(rng, deg, kinds)
    assert g.new == new
    g.n_id = np.concatenate([g.seeds, g.fresh_ids])
    stored = rng.integers(0, 4, len(g.rowptr) - 1)          # entries per feature row
    for a, b in seam_tiles(nodes):
        if b - a > 1:
            stored[g.n_id[a]] = 0
        stored[g.n_id[b - 1]] = 3
    g.x = (np.arange(3)[None, :] < stored[:, None]) * rng.integers(1, 9, (len(stored), 3)).astype(np.float32)
    g.x = np.ascontiguousarray(g.x[:, rng.permutation(3)], np.float32)
    g.nodes, g.stored = nodes, stored
    return g
