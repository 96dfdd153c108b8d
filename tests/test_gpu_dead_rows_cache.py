"""Csr.has_dead_rows / Csr.dead_rows follow an in-place change of the value tensor (they are kept with its version
counter), and with them the partitioned GAT layer's all-reduced flag; facts handed in through with_facts stay as given."""
import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu


def _csr():
    from sgracex1_amd import ops
    rowptr = torch.tensor([0, 2, 3, 3 + 4, 8], dtype=torch.int32, device="cuda")
    col = torch.tensor([0, 1, 1, 0, 1, 2, 3, 3], dtype=torch.int32, device="cuda")
    val = torch.tensor([0.5, 1.0, 2.0, 0.25, 0.5, 1.0, 1.5, 3.0], dtype=torch.float16, device="cuda")
    return ops.Csr(rowptr, col, val, 4)


def test_dead_row_answers_follow_the_values():
    A = _csr()
    assert A.has_dead_rows is False and not A.dead_rows.any()
    assert A.has_dead_rows is False                                          # (the cached answer)
    A.val[3:7] = 0                                                           # row 2 loses every live entry, in place
    assert A.has_dead_rows is True
    assert A.dead_rows.tolist() == [False, False, True, False]
    A.val[4] = 1.0
    assert A.has_dead_rows is False and not A.dead_rows.any()


def test_given_facts_stay_as_given():
    A = _csr().with_facts(dead_row_mask=torch.zeros(4, dtype=torch.bool, device="cuda"), has_dead_rows=False)
    A.val[3:7] = 0
    assert A.has_dead_rows is False and not A.dead_rows.any()


def test_the_all_reduced_flag_flips_too(tmp_path):
    from sgracex1_amd import dist as D
    # (a file rendezvous: no port to collide on, nothing left in the environment)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rendezvous", rank=0, world_size=1)
    try:
        A = _csr()
        assert D.any_rank_has_dead_rows(A) is False
        A.val[3:7] = 0
        assert D.any_rank_has_dead_rows(A) is True
    finally:
        dist.destroy_process_group()
