"""The node evaluation head without a GPU: sgx_node_eval is declared, exported and bound under the unchanged version, every
argument error it documents answers before anything reaches a device, the numpy restatement the GPU test trusts
(tests/_node_eval_ref.py) agrees with torch's cross_entropy(reduction="sum") and argmax in float64 and holds the edge rules
-- a tie, NaN logits, a target outside the range, no selected row, a mask combined with a prefix -- and
train.NodeTrainer.capture_eval_loader refuses what it documents before it touches a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _node_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgx.h")


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared in include/sgx.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_symbols_are_declared_exported_and_bound(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_node_eval_workspace_bytes", "sgx_node_eval"):
        assert name in L.SYMBOLS
        assert re.search(r" T %s\b" % name, out), name
        assert len(getattr(L.lib, name).argtypes) == len(_declaration(name)), name
    assert L.lib.sgx_node_eval.restype is ctypes.c_int
    assert L.lib.sgx_node_eval_workspace_bytes.restype is ctypes.c_size_t
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+SGX_VERSION\s+(\d+)", text).group(1)) == 110 and L.lib.sgx_version() == 110
    assert int(re.search(r"#define\s+SGX_NODE_LOSS_ROWS\s+(\d+)", text).group(1)) == R.ROWS
    assert int(re.search(r"#define\s+SGX_NODE_LOSS_GRID\s+(\d+)", text).group(1)) == R.GRID
    assert R.ROW_COUNTS == [1, 15, 16, 17, 33, 8200]


def test_argument_errors_need_no_gpu(L):
    R.check_argument_errors(L.lib)


@pytest.mark.parametrize("n", [1, 17, 33, 100])
@pytest.mark.parametrize("P", R.WIDTHS)
@pytest.mark.parametrize("C", R.CLASSES)
@pytest.mark.parametrize("mask", R.MASKS)
def test_reference_against_torch(n, P, C, mask):
    case = R.make_case(n, P, C, mask=mask)
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    z32 = R.logits_f32(case["H"], case["W"], case["bias"])
    z64 = f64(case["H"]) @ f64(case["W"]).T + f64(case["bias"])
    e_z = R.gamma(P + 1) * (np.abs(case["H"]).astype(np.float64) @ np.abs(case["W"]).astype(np.float64).T
                            + np.abs(case["bias"]).astype(np.float64)) + R.TINY
    assert np.all(np.abs(z32.astype(np.float64) - z64.numpy()) <= e_z)        # the fmaf chain lies within gamma(P + 1) of float64
    assert np.array_equal(R.argmax_first(z32), torch.from_numpy(z32).argmax(1).numpy())
    t = torch.from_numpy(case["target"])
    for n_prefix in R.prefixes(n):
        (M, hits), loss, bound, z, _ = R.eval_ref(case["H"], case["W"], case["bias"], case["target"], case["mask"], n_prefix)
        assert np.array_equal(z.view(np.int32), z32.view(np.int32))
        sel = torch.arange(n) < n_prefix
        if case["mask"] is not None:
            sel &= torch.from_numpy(case["mask"])
        live = sel & (t >= 0) & (t < C)
        assert M == int(sel.sum()) and bound >= 0.0
        assert hits == int((live & (torch.from_numpy(z32).argmax(1) == t)).sum())
        # float64 on the fp32 logits: the reference's loss is torch's on the same operands
        want = float(F.cross_entropy(torch.from_numpy(z32).double()[live], t[live], reduction="sum")) if bool(live.any()) else 0.0
        assert abs(loss - want) <= 1e-12 * max(1.0, abs(want))
        if M == 0:
            assert (hits, loss, bound) == (0, 0.0, 0.0)
        # the bound is a small multiple of fp32's roundoff per row, not a chosen constant
        assert bound <= R.TINY + M * 64 * (C + 8) * R.U


def test_the_sums_order_is_two_level_over_blocks_of_rows():
    """On values whose double sum depends on the order, sum_in_order gives the stated one: rows inside a block first."""
    big, one = 2.0 ** 53, 1.0
    loss = np.zeros(2 * R.ROWS + 1)
    loss[0], loss[R.ROWS], loss[R.ROWS + 1], loss[2 * R.ROWS] = big, one, one, one
    sel = np.ones(loss.size, bool)
    # block 0: 2^53; block 1: 1 + 1 = 2; block 2: 1.  2^53 + 2 is exact and (2^53 + 2) + 1 is a tie that rounds to the even
    # 2^53 + 4; row by row from the left every + 1 is a tie that rounds back to 2^53
    assert R.sum_in_order(loss, sel) == big + 4.0
    assert float(np.cumsum(loss)[-1]) == big
    sel[R.ROWS + 1] = False                                  # an unselected row takes part in no sum: block 1 is 1, and lost
    assert R.sum_in_order(loss, sel) == big and R.sum_in_order(loss[:2 * R.ROWS], sel[:2 * R.ROWS]) == big
    sel[R.ROWS + 1], sel[0] = True, False
    assert R.sum_in_order(loss, sel) == 3.0
    assert R.sum_in_order(np.array([np.nan, 1.0]), np.array([False, True])) == 1.0
    rng = np.random.default_rng(0)
    v = rng.uniform(0, 3, 1000)
    assert abs(R.sum_in_order(v, np.ones(1000, bool)) - math.fsum(v)) <= 80 * R.U64 * math.fsum(v)


def test_edge_rules():
    # a tie: the lowest index wins, as torch's argmax
    case = R.make_tie_case()
    z = R.logits_f32(case["H"], case["W"], case["bias"])
    z64 = case["H"].astype(np.float64) @ case["W"].astype(np.float64).T + case["bias"]
    assert np.array_equal(z.astype(np.float64), z64)                 # integers: exact in any order
    assert np.array_equal(z[:, 2], z[:, 5]) and np.all(z[:, 2] > np.delete(z, (2, 5), axis=1).max(1))
    n = z.shape[0]
    (M, hits), loss, bound, _, _ = R.eval_ref(case["H"], case["W"], case["bias"], case["target"])
    assert (M, hits) == (n, (n + 1) // 2) and abs(loss - n * math.log(2.0)) <= 1e-9
    assert np.array_equal(R.argmax_first(z), torch.from_numpy(z).argmax(1).numpy())
    # NaN: at z[0] it counts as -inf, elsewhere it never wins; a row of NaN keeps index 0
    nan = np.float32(np.nan)
    zn = np.array([[nan, 1.0, 2.0], [3.0, nan, 2.0], [1.0, 2.0, nan], [nan, nan, nan], [nan, -np.inf, -np.inf]], np.float32)
    assert R.argmax_first(zn).tolist() == [2, 0, 1, 0, 0]
    # a target outside the range: no loss, no hit, nothing indexed, the row counts
    H = np.ones((4, 1), np.float32)
    W = np.array([[1.0], [2.0]], np.float32)
    for bad in (2, -1, 2 ** 40, -2 ** 40):
        (M, hits), loss, _, _, _ = R.eval_ref(H, W, None, np.array([1, bad, 1, 0]))
        assert (M, hits) == (4, 2) and abs(loss - (2 * math.log1p(math.exp(-1.0)) + math.log1p(math.exp(1.0)))) <= 1e-12
    # M == 0: by the prefix, by the mask, by both
    for mask, n_prefix in ((None, 0), (np.zeros(4, bool), None), (np.array([0, 0, 1, 1], bool), 2)):
        assert R.eval_ref(H, W, None, np.array([1, 1, 1, 0]), mask, n_prefix)[:3] == ((0, 0), 0.0, 0.0)
    # a mask combined with a prefix: both must hold; a prefix past the rows selects as the row count does
    mask = np.array([1, 0, 1, 1], np.uint8)
    assert R.eval_ref(H, W, None, np.array([1, 1, 0, 1]), mask, 3)[0] == (2, 1)
    assert R.eval_ref(H, W, None, np.array([1, 1, 0, 1]), mask, 9)[0] == R.eval_ref(H, W, None, np.array([1, 1, 0, 1]), mask, 4)[0] == (3, 2)
    # NaN in an unselected row reaches nothing
    Hn = H.copy()
    Hn[1] = np.nan
    a, b = R.eval_ref(Hn, W, None, np.array([1, 1, 0, 1]), mask, 4), R.eval_ref(H, W, None, np.array([1, 1, 0, 1]), mask, 4)
    assert a[:3] == b[:3] and math.isfinite(a[1])


def test_the_small_graph_gives_two_full_batches_and_a_short_one():
    x, ei, y, train, test = R.small_graph()
    assert x.shape == (R.N_NODES, R.N_FEATURES) and R.N_NODES <= 260 and ei.shape[0] == 2
    assert int(test.sum()) == R.N_TEST == 2 * R.BATCH + 6 and int(train.sum()) == R.N_TRAIN and not (train & test).any()
    assert int((x != 0).sum(1).max()) <= 64                          # what a padded loader asks of the feature rows
    assert set(np.unique(y)) == set(range(R.N_CLASSES))


class _Model(torch.nn.Module):
    """What NodeTrainer asks of a model, on the host."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 3)

    def features(self, x, edge_index):
        return x


def test_capture_eval_loader_refuses_what_it_documents():
    from types import SimpleNamespace
    from sgracex1_amd.train import NodeTrainer
    trainer = NodeTrainer(_Model())
    state = trainer.state()
    unpadded = SimpleNamespace(pad=False, padded_batch=lambda: None, y=torch.zeros(4, dtype=torch.int64))
    graph_loader = SimpleNamespace(pad=True, y=torch.zeros(4, dtype=torch.int64))          # a GraphLoader has no padded_batch
    unlabelled = SimpleNamespace(pad=True, padded_batch=lambda: None, y=None, transposed=False)
    for loader in (unpadded, graph_loader, [1, 2, 3]):
        with pytest.raises(ValueError, match=r"capture_eval_loader takes a NeighborLoader\(pad=True\)"):
            trainer.capture_eval_loader(loader)
    with pytest.raises(ValueError, match="capture_eval_loader: the loader's data carries no labels"):
        trainer.capture_eval_loader(unlabelled)
    with pytest.raises(ValueError, match=r"capture_loader takes a NeighborLoader\(pad=True\)"):
        trainer.capture_loader(unpadded)                             # the training twin's refusal keeps its words
    assert all(torch.equal(a, b) for a, b in zip(state, trainer.state())) and trainer.model.training
