"""Restatement of the neighbour-sampling rule of include/sgx.h in numpy / Python integers, for the sampler tests.

Reads only the rows it samples, so a host copy of a full-size CSR (rowptr, col as numpy arrays) is enough."""
import numpy as np

M64 = (1 << 64) - 1
SENTINEL = 0x7FFFFFFF


def mix64(z):
    """splitmix64 finaliser on Python ints."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hop_key(seed, step, hop):
    return mix64(mix64(mix64(seed) ^ (step & M64)) ^ hop)


def _mix64_np(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(key, v, deg, k):
    """t_j for j = deg-k .. deg-1 (vectorised): high word of mix64(key ^ mix64(v << 32 | j)) * (j + 1)."""
    j = np.arange(deg - k, deg, dtype=np.uint64)
    w = (np.uint64(v) << np.uint64(32)) | j
    r = _mix64_np(np.uint64(key) ^ _mix64_np(w))
    m = j + np.uint64(1)                                   # < 2^32: the 128-bit product's high word from 32-bit halves
    rh, rl = r >> np.uint64(32), r & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        hi = (rh * m + ((rl * m) >> np.uint64(32))) >> np.uint64(32)
    return hi.astype(np.int64)


def floyd(key, v, deg, k):
    """Positions (ascending) sampled from a row of `deg` entries with fan-out k."""
    if k < 0 or deg <= k:
        return list(range(deg))
    chosen = set()
    for j, t in zip(range(deg - k, deg), draws(key, v, deg, k).tolist()):
        chosen.add(j if t in chosen else t)
    return sorted(chosen)


def sample(rowptr, col, seeds, fanouts, seed=0, step=0):
    """-> n_id, out_rowptr, out_col, edge_pos, hop_nodes, hop_edges (numpy int64 / lists), or raises ValueError for
    repeated seeds."""
    seeds = [int(s) for s in seeds]
    if len(set(seeds)) != len(seeds):
        raise ValueError("repeated seed")
    local = {v: i for i, v in enumerate(seeds)}
    n_id = list(seeds)
    row_start = {}
    out_col, edge_pos = [], []
    hop_nodes, hop_edges = [len(seeds)], [0]
    f0, f1 = 0, len(seeds)
    for h, k in enumerate(fanouts):
        key = hop_key(seed, step, h)
        for i in range(f0, f1):
            v = n_id[i]
            p0, p1 = int(rowptr[v]), int(rowptr[v + 1])
            row_start[i] = len(out_col)
            for p in floyd(key, v, p1 - p0, k):
                c = int(col[p0 + p])
                if c not in local:
                    local[c] = len(n_id)
                    n_id.append(c)
                out_col.append(local[c])
                edge_pos.append(p0 + p)
        f0, f1 = f1, len(n_id)
        hop_nodes.append(len(n_id))
        hop_edges.append(len(out_col))
    out_rowptr = [row_start.get(i, len(out_col)) for i in range(len(n_id))] + [len(out_col)]
    return (np.asarray(n_id, np.int64), np.asarray(out_rowptr, np.int64), np.asarray(out_col, np.int64),
            np.asarray(edge_pos, np.int64), hop_nodes, hop_edges)


def sample_take_all(rowptr, col, seeds, n_hops):
    """sample(rowptr, col, seeds, [-1] * n_hops) -- or any fan-outs no row's degree exceeds -- in closed form: every
    frontier row keeps all its positions, so nothing is drawn and a hop is a handful of array operations.  For the
    frontiers of millions of rows that sample()'s loop over rows cannot walk.  Same six values, same ValueError."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    seeds = np.asarray(seeds, np.int64).reshape(-1)
    local = np.full(len(rowptr) - 1, -1, np.int64)         # node -> local id, -1 = not in n_id yet
    local[seeds] = np.arange(len(seeds))
    if (local[seeds] != np.arange(len(seeds))).any():
        raise ValueError("repeated seed")
    n_id, row_ends, out_col, edge_pos = [seeds], [], [], []
    hop_nodes, hop_edges = [len(seeds)], [0]
    frontier = seeds
    for _ in range(n_hops):
        deg = rowptr[frontier + 1] - rowptr[frontier]
        ends = np.cumsum(deg)
        # the ranges [rowptr[v], rowptr[v + 1]) of the frontier rows, one behind the other
        pos = np.repeat(rowptr[frontier] - (ends - deg), deg) + np.arange(int(deg.sum()))
        c = col[pos]
        fresh = c[local[c] < 0]
        first = np.sort(np.unique(fresh, return_index=True)[1])          # first appearance of every new node in the hop
        frontier = fresh[first]
        local[frontier] = hop_nodes[-1] + np.arange(len(frontier))
        n_id.append(frontier)
        row_ends.append(hop_edges[-1] + ends)
        out_col.append(local[c])
        edge_pos.append(pos)
        hop_nodes.append(hop_nodes[-1] + len(frontier))
        hop_edges.append(hop_edges[-1] + len(pos))
    # the rows of the nodes new at the last hop are empty
    out_rowptr = np.concatenate([np.zeros(1, np.int64)] + row_ends + [np.full(len(frontier), hop_edges[-1], np.int64)])
    return (np.concatenate(n_id), out_rowptr, np.concatenate(out_col), np.concatenate(edge_pos), hop_nodes, hop_edges)
