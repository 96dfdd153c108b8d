"""The rule of the attention gradient by stored entries (sgx_gat_attention_grad_flat, include/sgx.h) restated in numpy:
an fp32 emulation in the rule's order, the float64 value, and the error bound the rule's longest addition chain gives.
Plain numpy; nothing here touches the GPU.

With T = sgx_spmm_flat_chunk(), end = min(rowPtr[n_rows], nnz) and L = the power of two >= ceil(F / 4), at most 64:
the entries [0, end) are cut into chunks of T, the rows into chunks of T; inside a chunk group g of the 64 / L lane groups
takes items g, g + 64 / L, ... in ascending order, one fma per item and column onto +0; the groups' sums are added in
group order; the chunks' partial rows are added in 16 chains by chunk index (chain q: chunks q, q + 16, ...) from +0, and
the chains in order from +0.  Nothing at or behind `end` is read, so the capacity does not show in the result.

The emulation forms an fma as fp32(float64(s) * float64(w) + float64(t)): the product is exact, the sum is rounded to 53
bits before it is rounded to 24 -- not always the bits of a fused multiply-add, and inside the same bound."""
import numpy as np

FIN_CHAINS = 16


def lanes(F):
    L = 1
    while L < -(-F // 4):
        L *= 2
    return min(L, 64)


def depth(T, F, n_chunks):
    """the longest addition chain of an output element: inside a group + the groups + the second launch"""
    L = lanes(F)
    return T * L // 64 + 64 // L + -(-max(n_chunks, 1) // FIN_CHAINS) + FIN_CHAINS


def _fma(s, w, t):
    return (np.float64(s) * w.astype(np.float64) + t.astype(np.float64)).astype(np.float32)


def _half(idx, s, Wh, T):
    """one half in the rule's order: item k contributes s[k] * Wh[idx[k]]"""
    F = Wh.shape[1]
    groups = 64 // lanes(F)
    partials = []
    for lo in range(0, len(idx), T):
        hi = min(lo + T, len(idx))
        tot = None
        for g in range(groups):
            t = np.zeros(F, np.float32)
            for k in range(lo + g, hi, groups):
                t = _fma(s[k], Wh[idx[k]], t)
            tot = t if tot is None else (tot + t).astype(np.float32)
        partials.append(tot)
    chains = []
    for q in range(FIN_CHAINS):
        t = np.zeros(F, np.float32)
        for c in range(q, len(partials), FIN_CHAINS):
            t = (t + partials[c]).astype(np.float32)
        chains.append(t)
    out = np.zeros(F, np.float32)
    for t in chains:
        out = (out + t).astype(np.float32)
    return out


def emulate(rp, ci, sg, g1, Wh, T, capacity=None):
    """fp32 [2 F] by the rule.  ci / sg may hold a capacity's worth of entries: what lies at or behind `end` is not read."""
    Wh = np.asarray(Wh, np.float32)
    n = len(rp) - 1
    end = int(rp[-1]) if n > 0 else 0
    end = max(0, min(end, len(ci) if capacity is None else capacity))
    first = _half(np.arange(n), np.asarray(g1, np.float32), Wh, T)
    second = _half(np.asarray(ci[:end], np.int64), np.asarray(sg[:end], np.float32), Wh, T)
    return np.concatenate([first, second])


def exact(rp, ci, sg, g1, Wh):
    """(value, sum of |term|) in float64, [2 F] each"""
    Wh = np.asarray(Wh, np.float64)
    n = len(rp) - 1
    end = int(rp[-1]) if n > 0 else 0
    g1, s, c = np.asarray(g1, np.float64)[:n], np.asarray(sg, np.float64)[:end], np.asarray(ci[:end], np.int64)
    v = np.concatenate([(g1[:, None] * Wh[:n]).sum(0), (s[:, None] * Wh[c]).sum(0)])
    a = np.concatenate([(np.abs(g1)[:, None] * np.abs(Wh[:n])).sum(0), (np.abs(s)[:, None] * np.abs(Wh[c])).sum(0)])
    return v, a


def bound(rp, T, F, magnitude):
    """(d + 2) 2^-24 sum |term| per element, d the longest chain of its half: the entries' half counts the entry chunks,
    the rows' half the row chunks"""
    n = len(rp) - 1
    end = int(rp[-1]) if n > 0 else 0
    d_rows, d_ent = depth(T, F, -(-n // T)), depth(T, F, -(-end // T))
    d = np.concatenate([np.full(F, d_rows + 2.0), np.full(F, d_ent + 2.0)])
    return d * 2.0 ** -24 * magnitude


# ---- the graphs: name -> degrees, as functions of T ---------------------------------------------------------------------

def degree_cases(T):
    fill = lambda total, k=7: [k] * (total // k) + ([total % k] if total % k else [])
    return {
        "end_0": [0] * 5,
        "end_1": [0, 1, 0],
        "end_T-1": fill(T - 1),
        "end_T": fill(T),
        "end_T+1": fill(T + 1),
        "end_3T+5": fill(3 * T + 5),
        "hub": [3, 3 * T + 40, 5, 0, 9],                                       # a hub row over 3 T
        "empty_runs": [0] * 9 + fill(T // 2, 5) + [0] * 40 + fill(T, 6) + [0] * 11,
        "rows_below_T": fill(T + 30, 3)[:T - 20],                               # n_rows < T
        "rows_2T+3": ([2, 0, 1] * T)[:2 * T + 3],                               # n_rows = 2 T + 3: three row chunks
    }


def build(deg, n_cols, seed=0):
    """(rowptr, col, sg, g1) with values in (-1, 1)"""
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(deg) + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = rng.integers(0, n_cols, int(rp[-1])).astype(np.int32)
    sg = (rng.random(int(rp[-1])) * 2 - 1).astype(np.float32)
    g1 = (rng.random(len(deg)) * 2 - 1).astype(np.float32)
    return rp, ci, sg, g1
