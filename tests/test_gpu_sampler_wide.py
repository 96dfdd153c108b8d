"""The sampler's wide form on the GPU (csrc/sample.hip, sample_wide_kernel: fan-outs 65 .. 1024 on the whole wavefront)
against the restatement of the rule in tests/_sampler_ref.py, bit for bit: at the lane-count and chunk-count edges, first
in a sample and behind a large frontier, on either side of the cut to the one-lane path, at the capacity check, and
recorded and replayed through the padded batch call.  One seeded graph of 1 500 nodes serves every test."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N = 1500
KS = (65, 100, 127, 128, 129, 1023, 1024, 1025)               # every fan-out a test samples rows over
HUB, EMPTY, LOOPS = 0, 1, 2
FEEDERS = range(720, 735)                                      # rows of three entries that name the planted rows
SHAPE = -2


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def graph():
    """-> (Csr on the device, host rowptr, host col, planted: {k: rows of degree k+1, k+2, 2k, 3k+1, k, k-1}).  Ordinary
    rows have 3 to 40 entries; row HUB has 70 001, row EMPTY none, row LOOPS 131 with self loops and a repeated edge.  The
    FEEDERS have three entries each: between them every planted row of the fan-outs from 100 on, the hub, EMPTY and LOOPS,
    so that a first hop of fan-out 3 over them puts those rows into the frontier of the second."""
    from sgracex1_amd import graphs
    rng = np.random.default_rng(17)
    deg = rng.integers(3, 41, N)
    deg[HUB], deg[EMPTY], deg[LOOPS] = 70001, 0, 131
    planted, row = {}, 10
    for k in KS:
        planted[k] = list(range(row, row + 6))
        deg[row:row + 6] = (k + 1, k + 2, 2 * k, 3 * k + 1, k, k - 1)
        row += 6
    deg[FEEDERS.start:FEEDERS.stop] = 3
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, N, rowptr[-1])
    col[rowptr[LOOPS]:rowptr[LOOPS] + 6] = (LOOPS, LOOPS, 5, 5, 5, LOOPS)
    fed = [r for k in KS if k >= 100 for r in planted[k]] + [HUB, EMPTY, LOOPS]
    assert len(fed) == 3 * len(FEEDERS)
    col[rowptr[FEEDERS.start]:rowptr[FEEDERS.stop]] = fed
    A = graphs.csr_from_numpy(rowptr, col, np.ones(len(col), np.float32), N, dtype=torch.float32)
    return A, rowptr, col, planted


def seeds_of(feeders=False):
    """Every planted row, the hub, the empty row, the row of loops and a few ordinary ones, in a shuffled order; or, for
    a wide hop behind a first one, the feeders among 120 ordinary rows."""
    _, _, _, planted = graph()
    if feeders:
        return np.random.default_rng(6).permutation(list(FEEDERS) + list(range(800, 920)))
    rows = [HUB, EMPTY, LOOPS] + [r for k in KS for r in planted[k]] + list(range(700, 712))
    return np.random.default_rng(5).permutation(rows)


@functools.lru_cache(maxsize=None)
def reference(fanouts, seed, step):
    _, rowptr, col, _ = graph()
    return R.sample(rowptr, col, seeds_of(fanouts[0] < 64), list(fanouts), seed=seed, step=step)


def node_map():
    from sgracex1_amd import ops
    return ops._node_maps[(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)]


def check(fanouts, seed, step, seeds=None):
    from sgracex1_amd import ops
    A, rowptr, col, _ = graph()
    if seeds is None:
        want = reference(tuple(fanouts), seed, step)
        seeds = seeds_of(fanouts[0] < 64)
    else:
        want = R.sample(rowptr, col, seeds, fanouts, seed=seed, step=step)
    s = ops.sample_neighbors(A, torch.as_tensor(np.asarray(seeds, np.int64), device=DEV), fanouts, seed=seed, step=step)
    n_id, rp, oc, pos, hn, he = want
    assert s.hop_nodes == hn and s.hop_edges == he
    assert np.array_equal(s.n_id.cpu().numpy(), n_id)
    assert np.array_equal(s.adj.rowptr.cpu().numpy(), rp)
    assert np.array_equal(s.adj.col[:s.adj.nnz].cpu().numpy(), oc)
    assert np.array_equal(s.edge_pos.cpu().numpy(), pos)
    assert bool((node_map() == ops.SAMPLE_SENTINEL).all())
    return s


def test_graph_has_what_the_tests_need():
    from sgracex1_amd import ops
    _, rowptr, col, planted = graph()
    deg = np.diff(rowptr)
    assert deg[HUB] == 70001 and deg[EMPTY] == 0
    for k in KS:
        assert deg[planted[k]].tolist() == [k + 1, k + 2, 2 * k, 3 * k + 1, k, k - 1]
    loops = col[rowptr[LOOPS]:rowptr[LOOPS + 1]]
    assert (loops == LOOPS).sum() >= 3 and (loops == 5).sum() >= 3
    assert set(seeds_of().tolist()) >= {HUB, EMPTY, LOOPS} | {r for k in KS for r in planted[k]}
    assert [ops.sample_form(k) for k in KS] == [2] * 7 + [3]


@pytest.mark.parametrize("seed,step", [(11, 0), (2 ** 40 + 3, 2 ** 33 + 1)])
@pytest.mark.parametrize("fanouts", [[65], [100], [127], [128], [129], [1023], [1024], [100, 3], [3, 100]],
                         ids=lambda f: "-".join(map(str, f)))
def test_wide_sample_equals_the_restatement(fanouts, seed, step):
    from sgracex1_amd import ops
    s = check(fanouts, seed, step)
    deg = np.diff(graph()[1])[s.n_id.cpu().numpy()]
    got = np.diff(s.adj.rowptr.cpu().numpy())
    for h, k in enumerate(fanouts):                            # every hop met rows over its fan-out, the wide ones included
        f0, f1 = (s.hop_nodes[h - 1] if h else 0), s.hop_nodes[h]
        assert np.array_equal(got[f0:f1], np.minimum(deg[f0:f1], k))
        assert (deg[f0:f1] > k).sum() >= (5 if ops.sample_form(k) == 2 else 1), (h, k)


def test_the_cut_to_the_one_lane_path():
    from sgracex1_amd import ops
    _, _, _, planted = graph()
    cut = ops.SAMPLE_WIDE_MAX
    assert (ops.sample_form(cut), ops.sample_form(cut + 1)) == (2, 3)
    over = planted[cut + 1][:4]                                # degrees cut + 2, cut + 3, 2 cut + 2, 3 cut + 4
    check([cut + 1], 3, 1, seeds=over)
    check([cut], 3, 1, seeds=over)


def test_capacity_one_below_the_bound_is_refused_and_the_map_refilled():
    from sgracex1_amd import _lib, ops
    A, _, _, _ = graph()
    check([100], 1, 0)                                         # the stream's map and workspace exist
    seeds = torch.as_tensor(seeds_of(), device=DEV).to(torch.int32)
    B, fan = seeds.numel(), (ctypes.c_int32 * 1)(100)
    mn, me = ctypes.c_int64(0), ctypes.c_int64(0)
    nbytes = _lib.lib.sgx_sample_workspace_bytes(N, A.nnz, B, 1, fan, ctypes.byref(mn), ctypes.byref(me))
    assert nbytes > 0 and me.value == B * 100
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=DEV)
    n_id, rowptr, col, pos = i32(mn.value), i32(mn.value + 1), i32(me.value), i32(me.value)
    hop_nodes, hop_edges = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
    m = node_map()

    def call(max_edges):
        return _lib.lib.sgx_sample_neighbors(A.rowptr.data_ptr(), A.col.data_ptr(), N, A.nnz, seeds.data_ptr(), B, 1, fan, 1, 0,
                                             m.data_ptr(), n_id.data_ptr(), rowptr.data_ptr(), col.data_ptr(), pos.data_ptr(),
                                             mn.value, max_edges, hop_nodes, hop_edges, ws.data_ptr(), nbytes,
                                             torch.cuda.current_stream().cuda_stream)

    assert call(me.value - 1) == SHAPE
    with pytest.raises(_lib.SgxError) as e:                    # the caller's part after an error that is not SGX_ERR_SEEDS
        ops._check_sample(SHAPE, m, "sgx_sample_neighbors")
    assert e.value.status == SHAPE and bool((m == ops.SAMPLE_SENTINEL).all())
    assert call(me.value) == 0
    want = reference((100,), 1, 0)
    E = hop_edges[1]
    assert [hop_nodes[1], E] == [want[4][1], want[5][1]]
    assert np.array_equal(pos[:E].cpu().numpy(), want[3]) and np.array_equal(col[:E].cpu().numpy(), want[2])
    assert bool((m == ops.SAMPLE_SENTINEL).all())


def test_recorded_padded_draws_equal_the_eager_draws():
    from sgracex1_amd import ops
    A, _, _, _ = graph()
    fan, seed = [100, 3], 7
    seeds = torch.as_tensor(seeds_of()[:32].copy(), device=DEV).to(torch.int32)
    cap = ops.node_pad_capacity(A, seeds.numel(), fan)
    buf = ops.NodePadBuffers(cap, N, torch.float32, DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    call = lambda: ops.sample_node_batch(A, seeds, fan, seed=seed, step=step, pad=cap, out=buf)
    eager = [ops.sample_node_batch(A, seeds, fan, seed=seed, step=t) for t in range(3)]
    assert (np.diff(graph()[1])[seeds.cpu().numpy()] > 100).sum() >= 5 and not same_bits(eager[0].edge_pos, eager[1].edge_pos)

    def equals_eager(p, u):
        n, E = u.n_id.numel(), u.edge_pos.numel()
        assert buf.counts[:2].tolist() == [n, E] and int(buf.status) == 0
        assert same_bits(p.n_id[:n], u.n_id) and bool((p.n_id[n:] == -1).all())
        assert same_bits(p.out_rowptr[:n + 1], u.adj.rowptr) and same_bits(p.out_col[:E], u.adj.col[:E])
        assert same_bits(p.edge_pos[:E], u.edge_pos)
        k = u.adj_norm.nnz
        assert same_bits(p.adj_norm.rowptr[:n + 1], u.adj_norm.rowptr)
        assert same_bits(p.adj_norm.col[:k], u.adj_norm.col[:k]) and same_bits(p.adj_norm.val[:k], u.adj_norm.val[:k])

    for t in range(3):                                         # three draws into one buffer set
        step.fill_(t)
        equals_eager(call(), eager[t])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                 # the side stream's workspace
    torch.cuda.current_stream().wait_stream(side)
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        p = call()
    for t in (2, 0, 1):
        step.fill_(t)
        graph_.replay()
        equals_eager(p, eager[t])
    assert bool((buf.node_map == ops.SAMPLE_SENTINEL).all())


def test_two_runs_at_1024_give_the_same_bytes():
    from sgracex1_amd import ops
    A, _, _, _ = graph()
    seeds = torch.as_tensor(seeds_of(), device=DEV)
    a = ops.sample_neighbors(A, seeds, [1024], seed=11, step=0)
    b = ops.sample_neighbors(A, seeds, [1024], seed=11, step=0)
    for x, y in ((a.n_id, b.n_id), (a.adj.rowptr, b.adj.rowptr), (a.adj.col, b.adj.col), (a.edge_pos, b.edge_pos)):
        assert same_bits(x, y)
    assert a.hop_nodes == b.hop_nodes and a.hop_edges == b.hop_edges
