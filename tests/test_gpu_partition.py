"""The partitioned layer 8 and 3 ways on the HIP kernels, in one process: every rank's halo plan comes from
dist.build_halo_plans_local (no process group), the exchange is simulated with ops.pack_rows and a concatenation, and every
rank's result is compared with the unpartitioned kernels (equal bits on rows the plan does not cut) and with float64 inside
the bounds of tests/_spmm_acc_ref.py (one pass: (n + 2) 2^-24 |A| @ |H| plus the rounding to the storage type; two passes:
the same with the first pass's fp32 sums as one more term).

Graphs of 4 000 rows (under 2^20 entries: every plan cuts rows over 64 entries): "uniform", degree ~10; "skewed": a third of
the rows empty, a few rows of 100..400 entries, one hub row with more than a quarter of all entries -- an nnz-balanced cut
into 8 leaves an empty partition behind it, and the hub goes through the plan's tasks -- and rows from 1 500 on that read
no column below their own, so the last partition of every cut reads its own rows only (no halo)."""
import functools

import numpy as np
import pytest
import torch

import _spmm_acc_ref as R

pytestmark = pytest.mark.gpu
TDT = {"f16": torch.float16, "f32": torch.float32}
N = 4000
U = 2.0 ** -24


def _uniform(dt):
    rng = np.random.default_rng(41)
    return R.random_rows(rng, rng.poisson(10.0, N), 0, N, dt)


def _skewed(dt):
    rng = np.random.default_rng(42)
    deg = rng.poisson(2.5, N)
    deg[rng.random(N) < 0.3] = 0
    deg[[100, 333, 700, 1200, 1450]] = [100, 400, 250, 180, 320]
    deg[40] = 3600                                                     # the hub
    deg = np.minimum(deg, N - np.arange(N))
    rp = np.zeros(N + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = np.empty(int(rp[-1]), np.int32)
    for i in np.nonzero(deg)[0]:
        first = i if i >= 1500 else 0                                  # from row 1500 on: no column below the row itself
        ci[rp[i]:rp[i + 1]] = first + np.sort(rng.choice(N - first, int(deg[i]), replace=False))
    va = R.rounded(rng.random(int(rp[-1])) * 2.0 - 0.7, dt)
    va[va == 0] = 0.5
    assert deg[40] > rp[-1] / 4
    return rp, ci, va


GRAPHS = {"uniform": _uniform, "skewed": _skewed}


@functools.lru_cache(maxsize=None)
def graph(gname, dt):
    return GRAPHS[gname](dt)


@functools.lru_cache(maxsize=None)
def table(dt):
    return R.table(np.random.default_rng(43), N, 64, dt)               # P = 41 takes its first 41 columns


@functools.lru_cache(maxsize=None)
def global_ref(gname, dt):
    return R.one_pass(graph(gname, dt), table(dt))


def _dev_csr(csr, n_cols, dt):
    from sgracex1_amd import ops
    rp, ci, va = csr
    return ops.Csr(torch.as_tensor(rp, dtype=torch.int32, device="cuda"), torch.as_tensor(ci, dtype=torch.int32, device="cuda"),
                   torch.as_tensor(va).to(TDT[dt]).cuda(), n_cols)


@functools.lru_cache(maxsize=None)
def global_csr(gname, dt):
    A = _dev_csr(graph(gname, dt), N, dt)
    assert A.wants_plan and A.plan.long_threshold == 64
    return A


@functools.lru_cache(maxsize=None)
def partition(gname, dt, world, cut):
    """bounds, every rank's (rowptr, col, val) on the device, the group-free halo plans, the request lists, and the float64
    sums of the own-partition edges and of the halo edges of every row"""
    from sgracex1_amd import dist as D
    A = global_csr(gname, dt)
    rp, ci, va = graph(gname, dt)
    bounds = D.row_partition(N, world, A.rowptr if cut == "nnz" else None)
    assert bounds[0] == 0 and bounds[-1] == N and all(a <= b for a, b in zip(bounds, bounds[1:]))
    parts = [D.slice_rows(A.rowptr, A.col, A.val, bounds[r], bounds[r + 1]) for r in range(world)]
    plans = D.build_halo_plans_local([p[1] for p in parts], bounds)
    need = [D.halo_requests(parts[r][1], bounds, r)[0] for r in range(world)]
    lo_of_row = np.repeat(np.array(bounds[:-1]), np.diff(bounds))
    hi_of_row = np.repeat(np.array(bounds[1:]), np.diff(bounds))
    rows = R.rows_of(rp)
    own = (ci >= lo_of_row[rows]) & (ci < hi_of_row[rows])
    H = table(dt)
    return dict(bounds=bounds, parts=parts, plans=plans, need=need, own=R.one_pass(R.subset((rp, ci, va), own), H),
                halo=R.one_pass(R.subset((rp, ci, va), ~own), H))


CASES = [(g, dt, w, c) for g in GRAPHS for dt in TDT for w in (8, 3) for c in ("rows", "nnz")]


@pytest.mark.parametrize("gname,dt,world,cut", CASES)
def test_halo_plans_remap_index_for_index(gname, dt, world, cut):
    S = partition(gname, dt, world, cut)
    bounds, plans, need = S["bounds"], S["plans"], S["need"]
    sizes = [b - a for a, b in zip(bounds, bounds[1:])]
    if gname == "skewed":
        assert any(sum(p.recv_counts) == 0 and p.n_own > 0 for p in plans)                   # a rank without a halo
        assert (0 in sizes) == (world == 8 and cut == "nnz")                                 # the empty partition
    for r, p in enumerate(plans):
        lo, hi = bounds[r], bounds[r + 1]
        col_global = S["parts"][r][1].long()
        table_rows = torch.cat([torch.arange(lo, hi, device="cuda")] + [need[r][g] for g in range(world)])
        assert p.n_own == hi - lo and p.n_table == table_rows.numel() and p.recv_counts == [t.numel() for t in need[r]]
        assert p.col_compact.dtype == torch.int32 and torch.equal(table_rows[p.col_compact.long()], col_global)
        off = 0
        for c in range(world):                                           # what consumer c asked this owner for
            seg = p.send_rows[off:off + p.send_counts[c]]
            assert torch.equal(seg, need[c][r] - lo) and p.send_counts[c] == plans[c].recv_counts[r]
            off += p.send_counts[c]
        assert off == p.send_rows.numel() and torch.equal(p.send_rows32.long(), p.send_rows)
        assert p.send_counts[r] == 0 and (p.send_rows >= 0).all() and (p.send_rows < max(1, hi - lo)).all()
    assert sum(sum(p.send_counts) for p in plans) == sum(sum(p.recv_counts) for p in plans)


def _tables(S, Hd):
    """the exchange in one process: every owner packs the rows its consumers asked for, every consumer's compact table is
    its own rows followed by the segments the owners packed for it, in owner order"""
    from sgracex1_amd import ops
    bounds, plans = S["bounds"], S["plans"]
    world = len(plans)
    packed = [ops.pack_rows(Hd[bounds[r]:bounds[r + 1]], plans[r].send_rows32) for r in range(world)]
    tables = []
    for c in range(world):
        segs = [Hd[bounds[c]:bounds[c + 1]]]
        for o in range(world):
            off = sum(plans[o].send_counts[:c])
            segs.append(packed[o][off:off + plans[o].send_counts[c]])
        tables.append(torch.cat(segs).contiguous())
    return packed, tables


@pytest.mark.parametrize("P", [64, 41])
@pytest.mark.parametrize("gname,dt,world,cut", CASES)
def test_partitioned_aggregation(gname, dt, world, cut, P):
    from sgracex1_amd import dist as D, ops
    S = partition(gname, dt, world, cut)
    bounds, plans, need = S["bounds"], S["plans"], S["need"]
    Hn = table(dt)[:, :P]
    Hd = torch.as_tensor(Hn).to(TDT[dt]).cuda().contiguous()
    A = global_csr(gname, dt)
    single = ops.spmm(A, Hd, relu=True)
    s, scale, n = (x[..., :P] if x.ndim == 2 else x for x in global_ref(gname, dt))
    want1, bound1 = R.finished(s, R.partial_bound(n, scale), dt, True)
    R.assert_within("unpartitioned", single.double().cpu().numpy(), want1, bound1)
    uncut_all = torch.as_tensor(n <= 64, device="cuda")
    (s_own, scale_own, n_own), (s_halo, scale_halo, n_halo) = (tuple(x[..., :P] if x.ndim == 2 else x for x in S[k])
                                                               for k in ("own", "halo"))
    packed, tables = _tables(S, Hd)
    hub_through_tasks = own_long = far_long = False
    for r, p in enumerate(plans):
        lo, hi = bounds[r], bounds[r + 1]
        rp, ci, va = S["parts"][r]
        table_rows = torch.cat([torch.arange(lo, hi, device="cuda")] + [need[r][g] for g in range(world)])
        assert packed[r].shape == (sum(p.send_counts), P) and tables[r].shape == (p.n_table, P)
        assert torch.equal(tables[r], Hd[table_rows])
        uncut = uncut_all[lo:hi]
        sl = slice(lo, hi)
        # all-gather form (global columns, the whole H) and one-pass halo form (compact columns, the compact table)
        adj_local, adj_compact = ops.Csr(rp, ci, va, N), ops.Csr(rp, p.col_compact, va, p.n_table)
        one_pass = {}
        for name, adj, tab in (("allgather", adj_local, Hd), ("halo", adj_compact, tables[r])):
            assert adj.plan.long_threshold == 64
            hub_through_tasks |= adj.plan.long_rows > 0 and int(n[sl].max(initial=0)) > 1000
            for use_plan in (True, False):
                got = ops.spmm(adj, tab, relu=True, use_plan=use_plan)
                assert got.shape == (hi - lo, P)
                assert torch.equal(got[uncut], single[sl][uncut]), (name, r, use_plan)
                R.assert_within(f"{name} rank {r}", got.double().cpu().numpy(), want1[sl], bound1[sl])
                one_pass[name, use_plan] = got
        # two-pass form: own-partition edges into fp32 partials, then the halo edges from the received rows
        own, far = D.split_own_halo(rp, p.col_compact, va, p.n_own)
        n_far = sum(p.recv_counts)
        A_own, A_far = ops.Csr(*own, p.n_own), ops.Csr(*far, n_far)
        assert A_own.nnz + A_far.nnz == ci.numel()
        part = ops.spmm_acc(A_own, tables[r][:p.n_own], partial_out=True, use_plan=False)
        two = ops.spmm_acc(A_far, tables[r][p.n_own:], relu=True, acc_in=part, use_plan=False)
        assert part.shape == (hi - lo, P) and two.shape == (hi - lo, P) and part.dtype == torch.float32
        acc = part.double().cpu().numpy()
        R.assert_within(f"partial rank {r}", acc, s_own[sl], R.partial_bound(n_own[sl], scale_own[sl]))
        R.assert_within(f"two-pass rank {r}", two.double().cpu().numpy(),
                        *R.finished(acc + s_halo[sl], R.partial_bound(n_halo[sl], np.abs(acc) + scale_halo[sl]), dt, True))
        no_halo_edge = torch.as_tensor(n_halo[sl] == 0, device="cuda")
        assert torch.equal(two[no_halo_edge], one_pass["halo", False][no_halo_edge])
        # ... and as the partitioned layer's backend runs it (use_plan=True) once both halves carry a plan: a hub row of the
        # own edges through the plan's tasks and spmm_split_finalize_kernel with acc_out, the thin halo half at its own CPL
        assert A_own.plan.long_threshold == 64 and A_far.plan.long_threshold == 64
        part_p = ops.spmm_acc(A_own, tables[r][:p.n_own], partial_out=True)
        two_p = ops.spmm_acc(A_far, tables[r][p.n_own:], relu=True, acc_in=part_p)
        acc_p = part_p.double().cpu().numpy()
        R.assert_within(f"planned partial rank {r}", acc_p, s_own[sl], R.partial_bound(n_own[sl], scale_own[sl]))
        R.assert_within(f"planned two-pass rank {r}", two_p.double().cpu().numpy(),
                        *R.finished(acc_p + s_halo[sl], R.partial_bound(n_halo[sl], np.abs(acc_p) + scale_halo[sl]), dt, True))
        assert torch.equal(part_p[uncut], part[uncut]) and torch.equal(two_p[uncut], two[uncut])
        assert torch.equal(two_p[no_halo_edge & uncut], one_pass["halo", True][no_halo_edge & uncut])
        own_long |= A_own.plan.long_rows > 0
        far_long |= A_far.plan.long_rows > 0
        if hi == lo:                                                     # the empty partition: the dense stage too
            X0 = torch.empty((0, 24), dtype=TDT[dt], device="cuda")
            Wt = torch.ones((P, 24), dtype=TDT[dt], device="cuda")
            assert ops.xw_dense(X0, Wt).shape == (0, P) and ops.col_sums(Hd[lo:hi]).tolist() == [0.0] * P
    if gname == "skewed":
        # the hub's halo half is cut in every partition of it, its own half where the partition is wide enough (row cuts)
        assert hub_through_tasks and far_long and (own_long or cut == "nnz")


@functools.lru_cache(maxsize=4)
def gat_case(gname, dt, P):
    """One graph with every 97th row's values zeroed, one-hot features, weights and attention: the single-GPU layer's
    result and the float64 restatement of tests/_gat_ref.py with its bounds (dead rows aside: their rule is the caller's)."""
    import _gat_ref as G
    from sgracex1_amd import ops
    M = 128
    A = global_csr(gname, dt)
    zeroed = torch.zeros(N, dtype=torch.bool, device="cuda")
    zeroed[torch.arange(3, N, 97, device="cuda")] = True
    rows_all = torch.repeat_interleave(torch.arange(N, device="cuda"), A.rowptr.diff().long())
    val2 = torch.where(zeroed[rows_all], torch.zeros_like(A.val), A.val)
    A2 = ops.Csr(A.rowptr, A.col, val2, N)
    dead = A2.dead_rows
    assert A2.has_dead_rows and bool((dead & zeroed).sum() >= 30)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5 + P)
    # one-hot feature rows: X . W is a row of W exactly, whatever the dense kernel's tile and summation order
    X = torch.zeros((N, M), dtype=TDT[dt], device="cuda")
    X[torch.arange(N, device="cuda"), torch.randint(0, M, (N,), generator=gen, device="cuda")] = 1
    Wt = ((torch.rand((P, M), generator=gen, device="cuda") - 0.5) / 2).to(TDT[dt])
    att = ((torch.rand(2 * P, generator=gen, device="cuda") - 0.5) / 2).to(TDT[dt])
    H_all = ops.xw_dense(X, Wt)
    assert H_all.stride(0) == ops.table_pitch(P, H_all.element_size())
    g = dict(rowptr=A.rowptr.cpu().numpy(), col=A.col.cpu().numpy(), val=val2.double().cpu().numpy(),
             Wh=H_all.double().cpu().numpy(), att=att.double().cpu().numpy())
    ref = G.forward(g, 1, relu=True, dead_rule="zero", out=dt)
    assert np.array_equal(ref["dead"], dead.cpu().numpy())
    return dict(A2=A2, val2=val2, dead=dead, X=X, Wt=Wt, att=att, H_all=H_all, ref=ref)


@pytest.mark.parametrize("P", [64, 41])
@pytest.mark.parametrize("gname,dt,world,cut", CASES)
def test_partitioned_gat_with_dead_rows(gname, dt, world, cut, P):
    """every 97th row loses its values: the mean row of ALL nodes is the sum of the ranks' column sums.  Live rows: inside
    the float64 bounds of tests/_gat_ref.py as the kernels choose their form, and the bits of the single-GPU layer where
    both run the same form (see _same_form); dead rows: relu(mean of Wh's rows) inside the bound _gat_ref.py states for
    that rule ((n + 2) 2^-24 mean |Wh| and the rounding to the storage type).  The table is pitched as X . W leaves it
    (P = 41: 64 halves / 44 floats)."""
    import _gat_ref as G
    from sgracex1_amd import _lib, ops
    S = partition(gname, dt, world, cut)
    bounds, plans = S["bounds"], S["plans"]
    A = global_csr(gname, dt)
    C = gat_case(gname, dt, P)
    A2, val2, dead, X, Wt, att, H_all, ref = (C[k] for k in ("A2", "val2", "dead", "X", "Wt", "att", "H_all", "ref"))
    assert sum(bool(dead[bounds[r]:bounds[r + 1]].any()) for r in range(world)) >= 3
    with _lib.tuning(**_same_form(P)):
        want = ops.layer_forward(A2, X, Wt, relu=True, gat_attention=att)
    H_r = [ops.xw_dense(X[bounds[r]:bounds[r + 1]], Wt) for r in range(world)]
    assert all(torch.equal(H_r[r], H_all[bounds[r]:bounds[r + 1]]) and H_r[r].shape == (bounds[r + 1] - bounds[r], P)
               for r in range(world))
    sums = torch.zeros(P, dtype=torch.float32, device="cuda")
    for r in range(world):
        sums += ops.col_sums(H_r[r])                                       # (the all-reduce, in rank order)
    H64 = H_all.double().cpu().numpy()
    err = np.abs(sums.double().cpu().numpy() - H64.sum(0))
    assert (err <= (N + 8) * U * np.abs(H64).sum(0)).all(), err.max()
    fill_row = sums / float(N)
    mean = np.maximum(H64.mean(0), 0.0)
    bound = (N + 2) * U * np.abs(H64).mean(0)
    bound = bound + (mean + bound) * G.OUT_U[dt] + G.OUT_SUB[dt]
    pitch = H_all.stride(0)
    packed = [ops.pack_rows(H_r[r], plans[r].send_rows32) for r in range(world)]
    names = {}
    for c, p in enumerate(plans):
        lo, hi = bounds[c], bounds[c + 1]
        buf = torch.full((p.n_table, pitch), 9.0, dtype=TDT[dt], device="cuda")     # rows pitched as X . W leaves them
        tab = buf[:, :P]
        tab[:p.n_own] = H_r[c]
        off = p.n_own
        for o in range(world):
            k = plans[o].send_counts[c]
            first = sum(plans[o].send_counts[:c])
            tab[off:off + k] = packed[o][first:first + k]
            off += k
        assert off == p.n_table
        rp, ci, va = S["parts"][c]
        adj = ops.Csr(rp, p.col_compact, val2[int(A.rowptr[lo]):int(A.rowptr[hi])].contiguous(), p.n_table)
        adj.plan                                                             # the planned forms, as the single-GPU layer runs
        kw = dict(relu=True, fill_dead_rows=False, fill_row=fill_row, n_nodes=N)
        got = ops.gat_aggregate(adj, tab, att, **kw)                         # the form the kernels choose for this partition
        assert got.shape == (hi - lo, P)
        d = dead[lo:hi]
        live = (~d).cpu().numpy()
        G.check(f"live rows of rank {c}", got.double().cpu().numpy()[live], ref["D"][lo:hi][live], ref["bD"][lo:hi][live],
                np.arange(lo, hi)[live], names)
        with _lib.tuning(**_same_form(P)):
            same = ops.gat_aggregate(adj, tab, att, **kw)
        assert torch.equal(same[~d], want[lo:hi][~d]), (c, int((same[~d] != want[lo:hi][~d]).any(1).sum()))
        for out in (got, same):
            assert (buf[:, P:] == 9.0).all()
            if bool(d.any()):
                g64 = out[d].double().cpu().numpy()
                assert (np.abs(g64 - mean[None, :]) <= bound[None, :]).all(), np.abs(g64 - mean[None, :]).max()


def _same_form(P):
    """Tuning under which the single-GPU layer and every partition run the SAME form of the aggregate, so that a live
    row's bits can be compared.  P = 64 takes the one-walk form on any plan.  P = 41 (a head that is no whole number of
    16-byte chunks) takes the two-stage form, whose first stage walks the short rows per row or as a scan in entry order
    -- chosen from the plan's degree order, which differs between the whole graph and a partition of it, and the two sum
    a row's exponentials in different orders: there the per-row walk is forced on both sides."""
    return {} if P == 64 else {"SGX_GAT_SCAN": "0"}
