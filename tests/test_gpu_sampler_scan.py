"""The three-launch exclusive scan behind the neighbour sampler and the node-batch preparation (scan_launch in
csrc/sample_device.h) at its tile and round edges, through its four functors: RowCounts and FirstSeen (ops.sample_neighbors),
LoopMissing and FeatureRows (ops.sample_node_batch).  A workgroup scans a tile of 2048 items and one workgroup scans up to
1024 tile sums per round, so past 2048 * 1024 items that workgroup makes a second and a third round on a carried sum.  The
graphs of tests/_sampler_scan_graphs.py put an exact item count through one scan each (tests/test_sampler_cpu.py holds them
to it); with fan-out -1 nothing is drawn, and every output is compared bit for bit with the closed form
_sampler_ref.sample_take_all.  Everything here is integer and exact: no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import _sampler_ref as R
import _sampler_scan_graphs as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TILE = 2048
TOP = 2048 * 1024
SIZES = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, TOP - 1, TOP, TOP + 1, 2 * TOP + 1]
assert (TILE, TOP, SIZES) == (G.TILE, G.TOP, G.SIZES)

_BUILDERS = {"frontier": G.frontier_graph, "edges": G.edge_graph, "second_hop": G.second_hop_graph}


def _np(t):
    return t.cpu().numpy()


def _csr(g):
    from sgracex1_amd import graphs
    return graphs.csr_from_numpy(g.rowptr, g.col, np.ones(len(g.col), np.float32), len(g.rowptr) - 1, dtype=torch.float32)


@functools.lru_cache(maxsize=2)
def _expected(kind, size, n_hops):
    g = _BUILDERS[kind](size)
    return R.sample_take_all(g.rowptr, g.col, g.seeds, n_hops)


def _map_is_clear():
    from sgracex1_amd import ops
    node_map = ops._node_maps[(DEV.index if DEV.index is not None else torch.cuda.current_device(),
                               torch.cuda.current_stream().cuda_stream)]
    return bool((node_map == ops.SAMPLE_SENTINEL).all())


def _sample(g, fanouts, A=None):
    from sgracex1_amd import ops
    return ops.sample_neighbors(_csr(g) if A is None else A, torch.as_tensor(g.seeds, device=DEV), fanouts)


def _check(kind, size, n_hops=1):
    g = _BUILDERS[kind](size)
    s = _sample(g, [-1] * n_hops)
    n_id, rp, oc, pos, hn, he = _expected(kind, size, n_hops)
    assert s.hop_nodes == hn and s.hop_edges == he
    assert np.array_equal(_np(s.n_id), n_id)
    assert np.array_equal(_np(s.adj.rowptr), rp)
    assert np.array_equal(_np(s.adj.col[:s.adj.nnz]), oc)
    assert np.array_equal(_np(s.edge_pos), pos)
    assert s.adj.n_rows == len(n_id) and s.adj.nnz == len(oc)
    assert _map_is_clear()
    return g, s


@pytest.mark.parametrize("s", SIZES)
def test_take_all_frontier_sizes(s):
    """RowCounts over exactly s frontier rows (the FirstSeen scan behind it over about 1.5 s slots)."""
    g, out = _check("frontier", s)
    assert out.hop_nodes[0] == g.frontier == s and out.hop_edges[1] == g.edges and out.hop_nodes[1] == s + g.new


@pytest.mark.parametrize("s", SIZES)
def test_take_all_edge_counts(s):
    """FirstSeen over exactly s sampled edges."""
    g, out = _check("edges", s)
    assert out.hop_edges[1] == g.edges == s and out.hop_nodes == [g.frontier, g.frontier + g.new]


def test_second_hop_frontier_past_one_round():
    """RowCounts at hop 1 over TOP + 1 rows: the frontier begins behind the seeds and the hop's offsets behind hop 0's
    edges, both added inside emit and total, across a carry round."""
    g, out = _check("second_hop", TOP + 1, n_hops=2)
    assert out.hop_nodes[1] - out.hop_nodes[0] == g.new == TOP + 1 and out.hop_nodes[0] > 0 and out.hop_edges[1] > 0
    assert out.hop_edges[2] > out.hop_edges[1] and out.hop_nodes[2] > out.hop_nodes[1]


@pytest.mark.parametrize("k", [1, 2])
def test_clipped_counts_past_one_round(k):
    """Fan-out k under degrees {0, 1, 3} on a frontier of TOP + 1 rows: the rows over the fan-out count k.  Which positions
    such a row draws is not restated at this size (test_gpu_sampler.py compares the draw bit for bit); what does not depend
    on the draw is exact."""
    g = G.frontier_graph(TOP + 1, (0, 1, 3))
    s = _sample(g, [k])
    n_id, rp, oc, pos = _np(s.n_id).astype(np.int64), _np(s.adj.rowptr), _np(s.adj.col[:s.adj.nnz]), _np(s.edge_pos).astype(np.int64)
    B = len(g.seeds)
    assert B == TOP + 1 and np.array_equal(n_id[:B], g.seeds)
    deg = g.rowptr[g.seeds + 1] - g.rowptr[g.seeds]
    assert (deg > k).any()
    want = np.zeros(len(n_id) + 1, np.int64)
    np.cumsum(np.minimum(deg, k), out=want[1:B + 1])
    want[B + 1:] = want[B]                                  # the rows of the nodes the hop found are empty
    assert np.array_equal(rp, want)
    assert s.hop_edges == [0, want[B]] and s.hop_nodes == [B, len(n_id)] and len(pos) == len(oc) == want[B]
    row = np.repeat(np.arange(B), np.diff(want[:B + 1]))    # the frontier row of every sampled edge
    assert ((pos >= g.rowptr[g.seeds[row]]) & (pos < g.rowptr[g.seeds[row] + 1])).all()
    assert (np.diff(pos)[row[1:] == row[:-1]] > 0).all()    # strictly increasing inside a row: no position twice
    assert np.array_equal(g.col[pos], n_id[oc])
    assert len(np.unique(n_id)) == len(n_id)
    assert _map_is_clear()


@pytest.mark.parametrize("kind", ["frontier", "edges"])
def test_repeat_gives_the_same_bytes(kind):
    """No atomic lies on the scan's result path: a second call at TOP + 1 items returns the same tensors."""
    g = _BUILDERS[kind](TOP + 1)
    A = _csr(g)
    a, b = _sample(g, [-1], A), _sample(g, [-1], A)
    assert a.hop_nodes == b.hop_nodes and a.hop_edges == b.hop_edges
    for x, y in ((a.n_id, b.n_id), (a.adj.rowptr, b.adj.rowptr), (a.adj.col, b.adj.col), (a.edge_pos, b.edge_pos)):
        assert x.data_ptr() != y.data_ptr() and torch.equal(x, y)


@pytest.mark.parametrize("nodes", [TILE + 1, TOP + 1])
def test_node_batch_row_pointers(nodes):
    """LoopMissing and FeatureRows over exactly `nodes` sampled nodes: rowPtr_norm and rowPtr_fea, with the counts the batch
    reports, from the sampler outputs of the same call (the tests above check those)."""
    from sgracex1_amd import ops
    g = G.node_batch_graph(nodes)
    fea = ops.feature_csr(torch.as_tensor(g.x, device=DEV))
    s = ops.sample_node_batch(_csr(g), torch.as_tensor(g.seeds, device=DEV), [-1], features=fea)
    n_id, rp, oc = _np(s.n_id).astype(np.int64), _np(s.adj.rowptr).astype(np.int64), _np(s.adj.col[:s.adj.nnz])
    assert s.hop_nodes == [len(g.seeds), nodes] and np.array_equal(n_id, g.n_id) and len(rp) == nodes + 1
    # rowPtr_norm[i] = out_rowPtr[i] + the rows ahead of i that hold no entry on their own column
    row = np.repeat(np.arange(nodes), np.diff(rp))
    loop = np.zeros(nodes, bool)
    loop[row[oc == row]] = True
    assert loop.any() and not loop.all()
    want = rp.copy()
    want[1:] += np.cumsum(~loop)
    N = s.adj_norm
    assert np.array_equal(_np(N.rowptr), want) and N.nnz == want[-1] and N.n_rows == nodes
    # rowPtr_fea: the running sum of the lengths of the feature rows n_id
    rp_x, col_x = _np(fea.rowptr).astype(np.int64), _np(fea.col[:fea.nnz])
    lens = rp_x[n_id + 1] - rp_x[n_id]
    assert np.array_equal(lens, g.stored[n_id])
    want = np.zeros(nodes + 1, np.int64)
    np.cumsum(lens, out=want[1:])
    assert np.array_equal(_np(s.fea.rowptr), want) and s.fea.nnz == want[-1] and s.fea.n_rows == nodes
    # (and the rows those offsets place: the columns of the feature rows n_id, one behind the other)
    take = np.repeat(rp_x[n_id] - want[:-1], lens) + np.arange(want[-1])
    assert np.array_equal(_np(s.fea.col[:s.fea.nnz]), col_x[take])
    assert _map_is_clear()
