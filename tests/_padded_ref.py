"""The rule of the padded batches (include/sgx.h, "padded batches") restated in numpy, on the graphs of
tests/_graph_prep_ref.fixture() without its 150-row ring (which is over every plan's row budget): the capacity of a
(set, B) from the per-graph counts, and the arrays of a padded batch from the arrays of the unpadded one.
"""
import numpy as np

import _graph_prep_ref as P

N_SET = 7                                          # graphs 0 .. 6 of the fixture


def graphs():
    return P.fixture()[:N_SET]


def counts(gs=None):
    """Per graph: rows, stored edges, adjacency entries (repeated edges summed: distinct (row, col)), feature entries
    (non-zeros of x), normalised-adjacency entries (repeated edges kept, a loop added where none is stored)."""
    gs = graphs() if gs is None else gs
    rows = np.array([g["x"].shape[0] for g in gs], np.int64)
    edges = np.array([g["edge_index"].shape[1] for g in gs], np.int64)
    adj = np.array([len({(int(r), int(c)) for r, c in g["edge_index"].T}) for g in gs], np.int64)
    fea = np.array([int(np.count_nonzero(g["x"])) for g in gs], np.int64)
    norm = np.array([len(P.normalise_graph(g["edge_index"], g["x"].shape[0])[1]) for g in gs], np.int64)
    return rows, edges, adj, fea, norm


def capacity(cs, B, pad_rows=None):
    """The capacity by the rule's words, one line each."""
    rows, edges, adj, fea, norm = cs
    largest = lambda c: int(np.sort(c)[::-1][:B].sum())
    N = largest(rows) if pad_rows is None else int(pad_rows)
    n_min = int(np.sort(rows)[:B].sum())
    R_f = int(rows.max())
    F = -(-(N - n_min) // R_f)
    return dict(batch_size=B, n_rows=N, n_min=n_min, filler_rows=R_f, n_graphs=B + F, n_edges=largest(edges),
                nnz_fea=largest(fea), nnz_adj=largest(adj) + N - n_min, nnz_norm=largest(norm) + N - n_min)


def pad_pattern(rowptr, col, vals, n, N, cap):
    """A CSR's live arrays (rowptr [n+1], col [a], vals {name: [a]}) padded: filler row n + j holds the one entry
    (n + j, 1) at a + j; zeros up to the capacity."""
    a, Pn = len(col), N - n
    assert a + Pn <= cap
    rp = np.concatenate([rowptr[:n], a + np.arange(Pn + 1)]).astype(np.int32)
    c = np.zeros(cap, np.int32)
    c[:a], c[a:a + Pn] = col, n + np.arange(Pn)
    out = {}
    for k, v in vals.items():
        w = np.zeros(cap, v.dtype)
        w[:a], w[a:a + Pn] = v, 1
        out[k] = w
    return rp, c, out


def padded(live, cap, n_feat):
    """The padded batch of the unpadded batch `live` (numpy arrays under ops.Collated's names; adj_val / fea_val /
    norm_val dicts by dtype name; norm_* may be missing) at capacity `cap` (a dict as capacity() gives)."""
    B, N, G, R = cap["batch_size"], cap["n_rows"], cap["n_graphs"], cap["filler_rows"]
    n, E = live["x"].shape[0], live["edge_index"].shape[1]
    Pn = N - n
    assert len(live["y"]) == B and 0 <= Pn <= (G - B) * R and E <= cap["n_edges"]
    out = {}
    out["x"] = np.concatenate([live["x"], np.zeros((Pn, n_feat), np.float32)])
    ei = np.full((2, cap["n_edges"]), -1, np.int64)
    ei[:, :E] = live["edge_index"]
    out["edge_index"] = ei
    out["batch"] = np.concatenate([live["batch"], B + np.arange(Pn) // R]).astype(np.int64)
    out["y"] = np.concatenate([live["y"], np.zeros(G - B, np.int64)])
    out["graph_ptr"] = np.concatenate([live["graph_ptr"][:B], n + np.minimum(Pn, np.arange(G - B + 1) * R)]).astype(np.int32)
    out["adj_rowptr"], out["adj_col"], out["adj_val"] = pad_pattern(live["adj_rowptr"], live["adj_col"], live["adj_val"], n, N,
                                                                  cap["nnz_adj"])
    f = len(live["fea_col"])
    out["fea_rowptr"] = np.concatenate([live["fea_rowptr"][:n], np.full(Pn + 1, f)]).astype(np.int32)
    out["fea_col"] = np.concatenate([live["fea_col"], np.zeros(cap["nnz_fea"] - f, np.int32)])
    out["fea_val"] = {k: np.concatenate([v, np.zeros(cap["nnz_fea"] - f, v.dtype)]) for k, v in live["fea_val"].items()}
    if "norm_col" in live:
        out["norm_rowptr"], out["norm_col"], out["norm_val"] = pad_pattern(live["norm_rowptr"], live["norm_col"], live["norm_val"],
                                                                         n, N, cap["nnz_norm"])
        out["norm_dead"] = np.concatenate([live["norm_dead"], np.zeros(Pn, bool)])
    return out
