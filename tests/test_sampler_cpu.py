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
