"""The rule of the prepared graph loader (include/sgx.h, "shuffled graph mini-batches with prepared adjacencies")
restated in numpy, and the hand-made fixture its tests run on.

Rule: normalise every graph ON ITS OWN (sym_norm2 with fill = 0 and unit fp32 weights: a self loop of weight 0 for
every node without one, appended behind the stored edges; a stable sort by (row, col), repeated edges kept; value =
dis[row] * w * dis[col] with dis = deg^-0.5, inf -> 0, deg = the row sums), then build a batch by laying the graphs'
sorted entries one after another with the columns shifted by the graph's first row in the batch; quantise the values
(tests/_quant_ref.py::quantise_adj, the reference's own unsigned grid function); a row is dead where it holds no
positive value.  tests/test_graph_loader_prepared_cpu.py checks that this is, bit for bit, what sym_norm2 and a COO -> CSR
give on the concatenated batch -- the graph-locality claim the loader rests on.

The one elementwise function whose bits are the library's own, deg^-0.5, is torch's pow applied to each graph's degrees:
the claim is that it is elementwise, not how it rounds.
"""
import numpy as np
import torch

import _quant_ref as Q

N_FEAT = 7


def _undirected(pairs):
    a = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.concatenate([a, a[:, ::-1]]).T.copy()


def _graph(n, edge_index, label):
    x = np.zeros((n, N_FEAT), np.float32)
    x[np.arange(n), (np.arange(n) * 3 + label) % N_FEAT] = 1.0
    return {"x": x, "edge_index": np.asarray(edge_index, np.int64).reshape(2, -1), "y": label}


def fixture():
    """Eight graphs: 0 a single node without an edge; 1 two nodes and one undirected edge; 2 a path of 5; 3 a star of 9;
    4 a path 0-1-2-3-4 whose node 4 is tied to node 5 by an edge stored 21 times in each direction (every entry of row 5
    is 1 / sqrt(21 * 22), under half a step of the 1-bit grid and over half a step of the 2-, 4- and 8-bit ones); 5 a path
    of 3 whose middle node stores a self loop; 6 a path of 3 and an isolated node; 7 a ring of 150 rows, over every plan's
    row budget."""
    ring = np.arange(150)
    return [
        _graph(1, np.zeros((2, 0), np.int64), 0),
        _graph(2, _undirected([(0, 1)]), 1),
        _graph(5, _undirected([(0, 1), (1, 2), (2, 3), (3, 4)]), 0),
        _graph(9, _undirected([(0, k) for k in range(1, 9)]), 1),
        _graph(6, _undirected([(0, 1), (1, 2), (2, 3), (3, 4)] + [(4, 5)] * 21), 0),
        _graph(3, np.concatenate([_undirected([(0, 1), (1, 2)]), np.array([[1], [1]])], axis=1), 1),
        _graph(4, _undirected([(0, 1), (1, 2)]), 0),
        _graph(150, _undirected(list(zip(ring, (ring + 1) % 150))), 1),
    ]


CONNECTED = [1, 2, 3, 4, 5]                        # no 1-node graph, no isolated node: no dead row up to 2 bits
PERMUTATION = [5, 2, 7, 0, 4, 1, 6, 3]
BATCHES = ([list(range(8))[i:i + 3] for i in range(0, 8, 3)]            # identity order at batch 3: a partial last batch
           + [PERMUTATION[i:i + 3] for i in range(0, 8, 3)]
           + [[3, 1, 3, 4]]                                              # a graph id twice
           + [[7]]                                                       # the 150-row graph alone
           + [CONNECTED])


def torch_graphs():
    from sgracex1_amd import pyg_lite as G
    return [G.Graph(torch.as_tensor(g["x"]), torch.as_tensor(g["edge_index"]), torch.tensor([g["y"]])) for g in fixture()]


def normalise_graph(edge_index, n):
    """One graph's (rowptr [n+1], col, val fp32) by the rule."""
    row, col = edge_index
    has = np.zeros(n, bool)
    has[row[row == col]] = True
    missing = np.nonzero(~has)[0]
    row, col = np.concatenate([row, missing]), np.concatenate([col, missing])
    w = np.concatenate([np.ones(edge_index.shape[1], np.float32), np.zeros(len(missing), np.float32)])
    order = np.argsort(row * n + col, kind="stable")
    row, col, w = row[order], col[order], w[order]
    deg = np.zeros(n, np.float32)
    for r, v in zip(row, w):                                   # (integers: exact in any order)
        deg[r] += v
    with np.errstate(divide="ignore"):
        dis = torch.from_numpy(deg).pow(-0.5).numpy()
    dis[np.isinf(dis)] = 0
    val = (dis[row] * w * dis[col]).astype(np.float32)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
    return rowptr, col, val


def dead_rows(rowptr, val):
    return np.array([not (val[rowptr[i]:rowptr[i + 1]] > 0).any() for i in range(len(rowptr) - 1)])


def prepared_batch(graphs, ids, qcs=()):
    """The batch of graphs `ids` by the rule: dict(rowptr int32, col int32, val fp32, val16 fp16, dead bool, and per
    constants c in qcs: q[k] fp32 values, q_dead[k])."""
    per = [normalise_graph(g["edge_index"], g["x"].shape[0]) for g in graphs]      # once per dataset
    rowptr, cols, vals, off, ent = [0], [], [], 0, 0
    for i in ids:
        rp, c, v = per[i]
        rowptr += list(ent + rp[1:])
        cols.append(c + off)
        vals.append(v)
        off, ent = off + len(rp) - 1, ent + len(c)
    rowptr, val = np.asarray(rowptr, np.int64), np.concatenate(vals).astype(np.float32)
    out = dict(rowptr=rowptr.astype(np.int32), col=np.concatenate(cols).astype(np.int32), val=val,
               val16=val.astype(np.float16), dead=dead_rows(rowptr, val), q=[], q_dead=[])
    for c in qcs:
        q = Q.quantise_adj(val, c)
        out["q"].append(q)
        out["q_dead"].append(dead_rows(rowptr, q))
    return out
