"""What the tests of node batches for the quantised layers share (test_node_batch_quant_cpu.py,
test_gpu_node_batch_quant.py): the two small graphs in numpy, the seeds and fan-outs, the restatement of a prepared batch
(numpy sampler + the sym_norm2 rule) and the torch statement of a quantised adjacency's dead rows."""
import numpy as np
import torch

import _node_batch_ref as NB
import _sampler_ref as R

BATCH = 16
FANOUTS = ([3, 2], [-1])
SAMPLE_SEED, SAMPLE_STEP = 11, 1


def seeded_graph():
    """300 nodes, 0 .. 11 in-neighbours each from a seeded generator, with empty rows, stored loops, repeated edges and
    two rows past 64 entries (one a row every second node lists: entries whose degree product is large)."""
    rng = np.random.default_rng(42)
    n = 300
    rows = [list(rng.integers(0, n, rng.integers(0, 12))) for _ in range(n)]
    rows[0] = [0, 3, 3, 0, 5]
    rows[1] = []
    rows[3] = [7, 7, 7, 2]
    rows[5] = list(rng.integers(0, n, 150))
    rows[6] = [c for c in rng.integers(0, n, 90) if c != 6]
    for r in range(10, n, 2):
        rows[r].append(5)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    return rowptr, np.asarray([c for r in rows for c in r], np.int64)


def seeded_weights(nnz):
    """Edge weights of the seeded graph: multiples of 1/8 in [1/8, 2], so that every degree is exact in fp32 and the
    small ones fall under the 1-bit grid's first step even on rows of four entries."""
    return (np.random.default_rng(1).integers(1, 17, nnz) / 8).astype(np.float32)


def hub_graph():
    """The graph of test_gpu_node_batch.py::_hub_graph: a hub of degree over 2^16, isolated nodes, self loops, repeated
    edges."""
    rng = np.random.default_rng(0)
    n = 1000
    rows = [list(rng.integers(0, n, rng.integers(0, 30))) for _ in range(n)]
    rows[0] = list(rng.integers(0, n, 70000))
    rows[7] = []
    rows[8] = []
    rows[9] = [9, 9, 9, 3, 3, 10]
    rows[10] = [9, 11, 0]
    rows[11] = [10, 10]
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    return rowptr, np.asarray([c for r in rows for c in r], np.int64)


GRAPHS = {"seeded": seeded_graph, "hub": hub_graph}
# 16 seeds each: the special rows first
SEEDS = {"seeded": [0, 1, 3, 5, 6, 10, 12, 14] + [31, 64, 97, 130, 163, 196, 229, 262],
         "hub": [0, 7, 9, 10, 11, 8, 500] + [100, 200, 300, 400, 600, 700, 800, 900, 999]}
# Where a LIVE row can lose an entry to the 1-bit grid (first step at 0.05): an entry w / sqrt(deg_r deg_c) with
# deg_r deg_c > 400 w^2.  On unit weights under fan-outs [3, 2] no degree passes 4, so the hub graph shows it under [-1]
# only (row 10 lists the hub); the seeded graph's weights of 1/8 show it under both.
LOSES = {("seeded", 0): True, ("seeded", 1): True, ("hub", 0): False, ("hub", 1): True}


def weights_of(name, nnz):
    return seeded_weights(nnz) if name == "seeded" else None


def restated_batch(rowptr, col, seeds, fanouts, fill, weights=None, seed=SAMPLE_SEED, step=SAMPLE_STEP):
    """The normalised adjacency of the prepared batch by the rules of include/sgx.h -> rowptr, col, fp32 values."""
    _, rp, oc, pos, _, _ = R.sample(rowptr, col, seeds, fanouts, seed=seed, step=step)
    w = None if weights is None else np.asarray(weights)[pos]
    q_ptr, q_col, q_val, _, _, _ = NB.sym_norm2_csr(rp, oc, w, fill)
    return q_ptr, q_col, q_val


def rows_of(rowptr):
    """The row of every stored entry (int64 tensor where rowptr lives)."""
    rowptr = torch.as_tensor(rowptr)
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), (rowptr[1:] - rowptr[:-1]).long())


def dead_rows(values, row, n):
    """bool [n]: the rows that hold no value > 0 -- (row-wise any(values > 0)) == False."""
    live = torch.zeros(n, dtype=torch.int64, device=values.device)
    live.index_add_(0, row, (values > 0).to(torch.int64))
    return live == 0
