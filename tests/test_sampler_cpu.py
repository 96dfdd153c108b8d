"""The neighbour-sampling rule of include/sgx.h as restated in tests/_sampler_ref.py (no GPU): Floyd's subset without
replacement, every position when the degree is at most the fan-out, the relabel order on hand-made graphs, uniformity
on a star; and the argument checks of the two new C entry points, which answer before touching a GPU."""
import ctypes
import math

import numpy as np
import pytest

import _sampler_ref as R


def _csr(n, edges):
    """CSR on the targets: row v = the sources j of the edges j -> v, in the order given."""
    rows = [[] for _ in range(n)]
    for j, v in edges:
        rows[v].append(j)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    return rowptr, np.asarray([c for r in rows for c in r], np.int64)


def test_vectorised_draws_equal_the_integer_statement():
    key = R.hop_key(7, 3, 1)
    for v, deg, k in ((0, 10, 3), (123456, 1 << 17, 64), (2_000_000, 3_000_000, 5)):
        j = np.arange(deg - k, deg)
        want = [(R.mix64(key ^ R.mix64((v << 32) | int(jj))) * (int(jj) + 1)) >> 64 for jj in j]
        got = R.draws(key, v, deg, k)
        assert got.tolist() == want
        assert (got >= 0).all() and (got <= j).all()


def test_floyd_is_without_replacement_and_ascending():
    for step in range(200):
        key = R.hop_key(1, step, 0)
        for deg, k in ((11, 10), (50, 10), (1000, 64), (300, 100)):
            s = R.floyd(key, 5, deg, k)
            assert len(s) == k and len(set(s)) == k
            assert s == sorted(s) and 0 <= s[0] and s[-1] < deg


def test_small_rows_and_minus_one_take_every_position():
    key = R.hop_key(0, 0, 0)
    assert R.floyd(key, 3, 7, 10) == list(range(7))
    assert R.floyd(key, 3, 10, 10) == list(range(10))
    assert R.floyd(key, 3, 500, -1) == list(range(500))
    assert R.floyd(key, 3, 0, 5) == []


def test_relabel_order_on_a_hand_made_graph():
    # edges j -> v; seeds [4, 0]; everything fits the fan-out, so the sample is the whole 2-hop neighbourhood
    edges = [(1, 4), (2, 4), (0, 4), (3, 0), (1, 0), (5, 1), (4, 1), (6, 2), (6, 3), (3, 3)]
    rowptr, col = _csr(7, edges)
    n_id, rp, oc, pos, hn, he = R.sample(rowptr, col, [4, 0], [5, 5])
    # hop 0: row 4 -> 1 2 0 (0 is a seed: id 1), row 0 -> 3 1;  new in order: 1 -> 2, 2 -> 3, 3 -> 4
    # hop 1: frontier 1 2 3: row 1 -> 5 4, row 2 -> 6, row 3 -> 6 3;  new: 5 -> 5, 6 -> 6
    assert n_id.tolist() == [4, 0, 1, 2, 3, 5, 6]
    assert hn == [2, 5, 7] and he == [0, 5, 10]
    assert rp.tolist() == [0, 3, 5, 7, 8, 10, 10, 10]
    assert oc.tolist() == [2, 3, 1, 4, 2, 5, 0, 6, 6, 4]
    assert [int(col[p]) for p in pos] == [int(n_id[c]) for c in oc]
    # a seed's self loop and a repeated edge are positions like any other
    rowptr, col = _csr(3, [(0, 0), (1, 0), (1, 0), (2, 1)])
    n_id, rp, oc, pos, hn, he = R.sample(rowptr, col, [0], [-1])
    assert n_id.tolist() == [0, 1] and oc.tolist() == [0, 1, 1] and rp.tolist() == [0, 3, 3]
    with pytest.raises(ValueError):
        R.sample(rowptr, col, [1, 1], [2])


def test_uniform_positions_on_a_star():
    """Degree 1000, k = 10, 5000 seeded draws (steps 0..4999): a chi-square test of the position counts (999 degrees of
    freedom, Wilson-Hilferty normal approximation), deterministic because the draws are."""
    deg, k, draws = 1000, 10, 5000
    counts = np.zeros(deg, np.int64)
    for step in range(draws):
        counts[R.floyd(R.hop_key(42, step, 0), 0, deg, k)] += 1
    assert counts.sum() == draws * k
    expect = draws * k / deg
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    dof = deg - 1
    z = ((chi2 / dof) ** (1 / 3) - (1 - 2 / (9 * dof))) / math.sqrt(2 / (9 * dof))
    p = 0.5 * math.erfc(z / math.sqrt(2))
    assert 0.001 < p < 0.999, (chi2, p)


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_sampler_argument_checks_need_no_gpu(L):
    lib = L.lib
    fan = (ctypes.c_int32 * 3)(15, 10, 5)
    mn, me = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.sgx_sample_workspace_bytes(1000, 5000, 10, 3, fan, ctypes.byref(mn), ctypes.byref(me)) > 0
    assert mn.value == min(1000, 10 + 150 + 1500 + 7500) and me.value == min(5000, 150 + 1500 + 7500)
    assert lib.sgx_sample_workspace_bytes(10**6, 10**7, 4, 2, (ctypes.c_int32 * 2)(3, 2), ctypes.byref(mn), ctypes.byref(me)) > 0
    assert (mn.value, me.value) == (4 + 12 + 24, 12 + 24)
    assert lib.sgx_sample_workspace_bytes(100, 500, 5, 1, (ctypes.c_int32 * 1)(-1), ctypes.byref(mn), ctypes.byref(me)) > 0
    assert (mn.value, me.value) == (100, 500)
    bad = [(1000, 5000, 10, 3, (ctypes.c_int32 * 3)(15, -2, 5)),      # fan-out below -1
           (1000, 5000, 10, 0, fan), (1000, 5000, 10, 65, fan),         # hops
           (1000, 5000, -1, 3, fan), (1000, 5000, 1001, 3, fan),         # batch
           (-1, 5000, 10, 3, fan), (1000, -5, 10, 3, fan), (1000, 1 << 31, 10, 3, fan),
           (1000, 5000, 10, 3, None)]
    for args in bad:
        assert lib.sgx_sample_workspace_bytes(*args, None, None) == 0, args

    fake = ctypes.c_void_p(0x1000)                    # never dereferenced: every call below fails its checks first
    hn, he = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()

    def call(fanouts=fan, n=1000, nnz=5000, batch=10, hops=3, rowptr=fake, col=fake, seeds=fake, node_map=fake,
             n_id=fake, out_rowptr=fake, out_col=fake, pos=fake, max_nodes=10**6, max_edges=10**6, hop_nodes=hn,
             ws=fake, ws_bytes=1 << 20):
        return lib.sgx_sample_neighbors(rowptr, col, n, nnz, seeds, batch, hops, fanouts, 0, 0, node_map, n_id,
                                        out_rowptr, out_col, pos, max_nodes, max_edges, hop_nodes, he, ws, ws_bytes, None)

    assert call(fanouts=None) == -1
    assert call(hop_nodes=None) == -1
    for name in ("rowptr", "col", "seeds", "node_map", "n_id", "out_rowptr", "out_col", "pos"):
        assert call(**{name: None}) == -1, name
    assert call(fanouts=(ctypes.c_int32 * 3)(15, -3, 5)) == -2
    assert call(hops=0) == -2
    assert call(batch=-1) == -2
    assert call(batch=1001) == -2
    assert call(n=-1) == -2
    assert call(max_nodes=999) == -2                                    # below the node bound (1000)
    assert call(max_edges=4999) == -2                                   # below the edge bound (5000)
    assert call(ws=None) == -4
    assert call(ws_bytes=16) == -4
    assert L.status_string(-8) != "unknown status"


# ---- the closed form for "every row keeps all its edges", and the graphs of tests/test_gpu_sampler_scan.py ------------
import _sampler_scan_graphs as G


def _same_sample(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype == np.int64 and np.array_equal(x, y)
    assert list(a[4]) == list(b[4]) and list(a[5]) == list(b[5])


@pytest.mark.parametrize("n_hops", [1, 2, 3])
def test_take_all_equals_the_row_loop(n_hops):
    # row v = the sources of the edges into v: empty rows (2, 8, 9), repeated edges (into 0 and 5), self loops (0, 3, 6),
    # seeds that neighbour each other (0, 1, 3), columns that point back at seeds from later hops (4 -> 0, 6 -> 1, 7 -> 3)
    edges = [(0, 0), (1, 0), (1, 0), (4, 0), (0, 1), (3, 1), (5, 1), (3, 3), (1, 3), (6, 3), (6, 3), (0, 4), (7, 4),
             (4, 5), (4, 5), (2, 5), (6, 6), (1, 6), (8, 6), (3, 7), (9, 7), (5, 7)]
    rowptr, col = _csr(10, edges)
    for seeds in ([0, 1, 3], [3, 0, 1], [2], [8, 2, 9], [5], [], list(range(9, -1, -1))):
        _same_sample(R.sample_take_all(rowptr, col, seeds, n_hops), R.sample(rowptr, col, seeds, [-1] * n_hops))
    # any fan-out no degree exceeds is the same sample (the largest degree here is 4)
    _same_sample(R.sample_take_all(rowptr, col, [0, 1, 3], n_hops), R.sample(rowptr, col, [0, 1, 3], [4] * n_hops, seed=3, step=9))
    with pytest.raises(ValueError):
        R.sample_take_all(rowptr, col, [1, 4, 1], n_hops)
    # random multigraphs, a third of the rows empty, and the scan graphs' builders at sizes the row loop can walk
    rng = np.random.default_rng(n_hops)
    for n in (1, 7, 60):
        deg = rng.integers(0, 6, n) * (rng.random(n) < 0.67)
        rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        c = rng.integers(0, n, rp[-1])
        seeds = rng.permutation(n)[:max(1, n // 4)]
        _same_sample(R.sample_take_all(rp, c, seeds, n_hops), R.sample(rp, c, seeds, [-1] * n_hops))
    for g in (G.frontier_graph(50), G.edge_graph(70), G.second_hop_graph(40), G.node_batch_graph(90, new=20)):
        _same_sample(R.sample_take_all(g.rowptr, g.col, g.seeds, n_hops), R.sample(g.rowptr, g.col, g.seeds, [-1] * n_hops))


def _hop0(g):
    """(degrees of the seeds' rows, first-appearance flags of their slots) from the arrays alone."""
    assert len(np.unique(g.seeds)) == len(g.seeds) and g.rowptr[0] == 0 and g.rowptr[-1] == len(g.col)
    assert (np.diff(g.rowptr) >= 0).all() and np.diff(g.rowptr).max() <= 3
    deg = g.rowptr[g.seeds + 1] - g.rowptr[g.seeds]
    c = np.concatenate([g.col[g.rowptr[v]:g.rowptr[v + 1]] for v in g.seeds.tolist()]) if len(g.seeds) < 5000 else None
    ends = np.cumsum(deg)
    slots = g.col[np.repeat(g.rowptr[g.seeds] - (ends - deg), deg) + np.arange(int(deg.sum()))]
    assert c is None or np.array_equal(c, slots)
    is_seed = np.zeros(len(g.rowptr) - 1, bool)
    is_seed[g.seeds] = True
    first = np.zeros(len(slots), bool)
    first[np.unique(slots, return_index=True)[1]] = True
    return deg, first & ~is_seed[slots]


@pytest.mark.parametrize("size", G.SIZES)
def test_scan_graphs_hold_the_item_counts_they_claim(size):
    """The cap on the degrees (3) and the exact item counts are what test_gpu_sampler_scan.py's sizes rest on."""
    g = G.frontier_graph(size)
    deg, flags = _hop0(g)
    assert g.frontier == len(g.seeds) == size and g.edges == deg.sum() and g.new == flags.sum()
    assert G.seams_hold(deg > 0) and G.seams_hold(flags)
    assert not np.array_equal(g.seeds, np.sort(g.seeds)) or size == 1
    g = G.edge_graph(size)
    deg, flags = _hop0(g)
    assert g.edges == deg.sum() == len(flags) == size and g.frontier == len(g.seeds) and g.new == flags.sum()
    assert G.seams_hold(flags)
    if size > 8:                                            # every kind of column that is not a first appearance
        ends = np.cumsum(deg)
        slots = g.col[np.repeat(g.rowptr[g.seeds] - (ends - deg), deg) + np.arange(size)]
        named = np.isin(slots, g.seeds)
        assert named.any() and (~named & ~flags).any() and (slots == np.repeat(g.seeds, deg)).any()


def test_scan_graphs_of_the_other_tests_hold_their_counts():
    top = G.TOP + 1
    g = G.second_hop_graph(top)
    deg, flags = _hop0(g)
    assert g.new == flags.sum() == top and g.edges == deg.sum() > 0 and g.frontier == len(g.seeds) > 0
    deg1 = np.diff(g.rowptr)[g.fresh_ids]                   # the rows of hop 1's frontier, in its order
    assert len(deg1) == top and G.seams_hold(deg1 > 0)
    g = G.frontier_graph(top, (0, 1, 3))
    deg, flags = _hop0(g)
    assert g.frontier == len(deg) == top and set(np.unique(deg)) == {0, 1, 3} and G.seams_hold(deg > 0)
    for k in (1, 2):                                        # rows over the fan-out in every seam tile, rows within it beside them
        assert G.seams_hold(deg > k)
    for nodes in (G.TILE + 1, top):
        g = G.node_batch_graph(nodes)
        deg, flags = _hop0(g)
        assert len(g.seeds) + flags.sum() == nodes == len(g.n_id) and np.array_equal(g.n_id[:len(g.seeds)], g.seeds)
        assert len(np.unique(g.n_id)) == nodes
        ends = np.cumsum(deg)
        slots = g.col[np.repeat(g.rowptr[g.seeds] - (ends - deg), deg) + np.arange(int(deg.sum()))]
        loop = np.zeros(nodes, bool)                        # sampled rows that hold a self loop (the found rows are empty)
        loop[np.repeat(np.arange(len(deg)), deg)[slots == np.repeat(g.seeds, deg)]] = True
        assert G.seams_hold(~loop) and loop.any()
        stored = (g.x != 0).sum(1)
        assert g.x.dtype == np.float32 and g.x.shape == (len(g.rowptr) - 1, 3) and set(np.unique(stored)) == {0, 1, 2, 3}
        assert G.seams_hold(stored[g.n_id] > 0)
        if nodes > G.TOP:                                   # empty feature rows on both sides of item TOP
            assert (stored[g.n_id[G.TOP - G.TILE:G.TOP]] == 0).any() and (stored[g.n_id[:G.TOP - G.TILE]] == 0).any()
