"""build_halo_plans_local -- every rank's halo plan in one process, without a collective -- gives, field by field, the plan
that build_halo_plan builds with its all-to-all of request lists in a 3-rank gloo group, on a graph with an nnz-balanced
cut, empty rows, a rank that needs nothing from another, and on an empty partition."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("col_compact", "send_rows", "send_rows32")


def _graph(n, seed):
    """the last third of the rows reads its own third only (no halo for the last rank of a 3-way row cut)"""
    rng = np.random.default_rng(seed)
    deg = rng.poisson(5.0, n)
    deg[rng.random(n) < 0.1] = 0
    deg[7] = 4 * n // 5                                                # a hub: the nnz-balanced cut moves
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(deg)
    lo = 2 * (n // 3)
    ci = np.concatenate([np.sort(rng.choice(np.arange(lo, n) if i >= lo else n, d, replace=False)) for i, d in enumerate(deg)])
    return torch.as_tensor(rp), torch.as_tensor(ci.astype(np.int32))


def _cases(n):
    from sgracex1_amd import dist as D
    rp, ci = _graph(n, 5)
    by_rows = D.row_partition(n, 3)
    return rp, ci, [by_rows, D.row_partition(n, 3, rp), [0, 0, n // 2, n]]        # ... and an empty first partition


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sgracex1_amd import dist as D
        rp, ci, cuts = _cases(301)
        for bounds in cuts:
            cols = [ci[int(rp[bounds[r]]):int(rp[bounds[r + 1]])] for r in range(world)]
            mine = D.build_halo_plan(cols[rank], bounds, rank)
            local = D.build_halo_plans_local(cols, bounds)[rank]
            assert (mine.bounds, mine.rank, mine.n_own, mine.n_table) == (local.bounds, local.rank, local.n_own, local.n_table)
            assert mine.send_counts == local.send_counts and mine.recv_counts == local.recv_counts
            for f in FIELDS:
                a, b = getattr(mine, f), getattr(local, f)
                assert a.dtype == b.dtype and torch.equal(a, b), (f, bounds)
        open(os.path.join(tmp, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_group_free_plans_equal_the_gloo_built_ones():
    port = 29100 + os.getpid() % 300
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(3, port, tmp), nprocs=3, join=True)
        assert all(os.path.exists(os.path.join(tmp, f"ok{r}")) for r in range(3))


def test_the_cases_are_what_they_claim():
    from sgracex1_amd import dist as D
    rp, ci, cuts = _cases(301)
    assert cuts[0] != cuts[1] and cuts[2][0] == cuts[2][1]
    cols = [ci[int(rp[cuts[0][r]]):int(rp[cuts[0][r + 1]])] for r in range(3)]
    plans = D.build_halo_plans_local(cols, cuts[0])
    assert sum(plans[2].recv_counts) == 0 and sum(plans[0].recv_counts) > 0          # a rank without a halo
    assert sum(sum(p.send_counts) for p in plans) == sum(sum(p.recv_counts) for p in plans)
    with pytest.raises(ValueError):
        D.build_halo_plans_local(cols[:2], cuts[0])
