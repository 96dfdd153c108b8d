"""Numpy restatement of the padded node batch rule (include/sgx.h, "padded node batches"): the capacity arithmetic from the
sampler's bounds, and the arrays that stand behind the live prefix of a batch -- filler rows, dealt spare entries, -1
tails -- built from the unpadded batch's arrays and counts.  Written from the header's text, independent of the kernels."""
import numpy as np


def bounds(n_nodes, nnz, batch, fanouts):
    """(max_nodes, max_edges) of a sample (include/sgx.h, "neighbour sampling"): per hop at most frontier * k edges, at
    most nnz; a frontier is at most what the graph holds beside the seeds."""
    front, nodes, edges = batch, batch, 0
    for k in fanouts:
        e = min(nnz if k < 0 else front * k, nnz)
        edges += e
        front = min(e, n_nodes - batch)
        nodes += front
    return min(nodes, n_nodes), min(edges, nnz)


def capacity(n_nodes, nnz, batch, fanouts, fea_rows=None):
    """N, C_a, C_f, E (and mn, me, F) by the rule."""
    mn, me = bounds(n_nodes, nnz, batch, fanouts)
    Cf = 0 if fea_rows is None else int(np.sort(np.asarray(fea_rows, np.int64))[::-1][:mn].sum())
    F = max(-(-me // 63), -(-Cf // 64))
    N = mn + F
    return dict(N=N, Ca=me + N, Cf=Cf, E=me, mn=mn, me=me, F=F)


def deal(start, rows, spare, per_row, base):
    """Row pointer entries [0 .. rows] of `rows` filler rows that begin at entry `start`, hold `base` entries each and take
    `spare` further entries, per_row to a row from row 0 on."""
    j = np.arange(rows + 1, dtype=np.int64)
    return start + base * j + np.minimum(spare, per_row * j)


def pad_batch(cap, n, edges, n_id, out_rowptr, out_col, edge_pos, rowptr_norm, col_norm, val_norm, dead, edge_index,
              edge_index_agg, rowptr_fea=None, col_fea=None, val_fea=None, y=None, masks=()):
    """The padded arrays of a batch given by its unpadded arrays (numpy, the live sizes).  -> dict of arrays."""
    N, Ca, Cf, E = cap["N"], cap["Ca"], cap["Cf"], cap["E"]
    a = int(rowptr_norm[n])
    P = N - n
    Sa = Ca - a - P
    assert 0 <= Sa <= 63 * P
    out = {}
    out["n_id"] = np.concatenate([n_id, np.full(P, -1, n_id.dtype)])
    out["out_rowptr"] = np.concatenate([out_rowptr[:n], np.full(P + 1, edges, out_rowptr.dtype)])
    tail = np.full(E - edges, -1, np.int32)
    out["out_col"] = np.concatenate([out_col[:edges], tail])
    out["edge_pos"] = np.concatenate([edge_pos[:edges], tail])
    ptr = deal(a, P, Sa, 63, 1)
    assert ptr[-1] == Ca and (np.diff(ptr) >= 1).all() and (np.diff(ptr) <= 64).all()
    out["rowptr_norm"] = np.concatenate([rowptr_norm[:n], ptr]).astype(np.int32)
    lens = np.diff(ptr)
    f_col = np.repeat(n + np.arange(P), lens)
    f_val = np.zeros(Ca - a, val_norm.dtype)
    f_val[ptr[:-1] - a] = 1
    out["col_norm"] = np.concatenate([col_norm[:a], f_col]).astype(np.int32)
    out["val_norm"] = np.concatenate([val_norm[:a], f_val])
    out["dead"] = np.concatenate([dead[:n], np.zeros(P, dead.dtype)])
    for name, ei in (("edge_index", edge_index), ("edge_index_agg", edge_index_agg)):
        full = np.full((2, E), -1, np.int64)
        full[:, :edges] = ei
        out[name] = full
    if rowptr_fea is not None:
        f = int(rowptr_fea[n])
        Sf = Cf - f
        assert 0 <= Sf <= 64 * P
        fptr = deal(f, P, Sf, 64, 0)
        assert fptr[-1] == Cf and (np.diff(fptr) <= 64).all()
        out["rowptr_fea"] = np.concatenate([rowptr_fea[:n], fptr]).astype(np.int32)
        out["col_fea"] = np.concatenate([col_fea[:f], np.zeros(Sf, np.int32)])
        out["val_fea"] = np.concatenate([val_fea[:f], np.zeros(Sf, val_fea.dtype)])
    if y is not None:
        out["y"] = np.concatenate([y[:n], np.zeros(P, y.dtype)])
    out["masks"] = [np.concatenate([m[:n], np.zeros(P, m.dtype)]) for m in masks]
    return out
