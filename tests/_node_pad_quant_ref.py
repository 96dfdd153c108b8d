"""Numpy restatement of the padded QUANTISED node batch rule (include/sgx.h, "padded node batches",
sgx_node_batch_sample_padded_quant): the unsigned-grid quantiser restated from sgrace._fq_unsigned in fp32 steps, and the
padded values_q / dead_row_q / values_lean of one constant set built from the unpadded quantised call's arrays and a
capacity.  Written from the header's text; it shares no code with the library."""
import numpy as np

F32 = np.float32


def fq(x, inv_scale, zero, qbits):
    """quantization_ufbits (SG.py:253-265) as the library evaluates it: the product inv_scale * x rounded to fp32, the sum
    with the zero point rounded to fp32, round half to even, the clip to 0 .. 2^qbits - 1, the division (exact)."""
    x = np.asarray(x, F32)
    t = (F32(inv_scale) * x).astype(F32) + F32(zero)
    q = np.clip(np.rint(t.astype(F32)), F32(0), F32(2 ** qbits - 1)).astype(F32)
    return (q / F32(2) if qbits == 1 else q / F32(2 ** (qbits - 1))).astype(F32)


def constants_of(qc):
    """(inv_scale, zero, qbits) as ops hands them to the C ABI: 1 / a_s formed in double and rounded to fp32."""
    return F32(1 / qc.a_s), F32(qc.a_z), int(qc.w_qbits)


def filler_lengths(n, a, N, Ca):
    """Entries of the P = N - n filler rows behind a live adjacency entries: one diagonal entry each and the S_a = C_a - a -
    P spare entries dealt 63 to a row from filler row 0 on."""
    P = N - n
    Sa = Ca - a - P
    assert 0 <= Sa <= 63 * P
    j = np.arange(P, dtype=np.int64)
    return 1 + np.clip(Sa - 63 * j, 0, 63)


def pad_quant(cap, n, rowptr_norm, val_norm, val_q, dead_q, lean, inv_scale, zero, qbits):
    """The padded arrays of one constant set.  cap: dict with N and Ca; n live rows; rowptr_norm [n + 1], val_norm / val_q /
    lean [a] and dead_q [n] of the UNPADDED quantised call (lean may be None).  -> dict(values_q [Ca] fp32, dead_row_q [N]
    bool, values_lean [Ca] fp32 or None).  The filler rows are formed by the rule, not copied: fq of the 1 or 0 values_norm
    holds there; dead where no quantised value is positive; the lean value of a dead row is its unquantised one."""
    N, Ca = cap["N"], cap["Ca"]
    a = int(rowptr_norm[n])
    lens = filler_lengths(n, a, N, Ca)
    assert a + int(lens.sum()) == Ca
    first = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    f_norm = np.zeros(Ca - a, F32)
    f_norm[first] = 1
    f_q = fq(f_norm, inv_scale, zero, qbits)
    row = np.repeat(np.arange(N - n), lens)
    f_live = np.zeros(N - n, np.int64)
    np.add.at(f_live, row, (f_q > 0).astype(np.int64))
    f_dead = f_live == 0
    out = {"values_q": np.concatenate([np.asarray(val_q[:a], F32), f_q]),
           "dead_row_q": np.concatenate([np.asarray(dead_q[:n], bool), f_dead]),
           "values_lean": None}
    if lean is not None:
        out["values_lean"] = np.concatenate([np.asarray(lean[:a], F32), np.where(f_dead[row], f_norm, f_q).astype(F32)])
    return out


def live_quant(n, rowptr_norm, val_norm, inv_scale, zero, qbits):
    """What the unpadded quantised call writes for a live batch, by the rule: (values_q, dead_row_q, values_lean)."""
    a = int(rowptr_norm[n])
    v = np.asarray(val_norm[:a], F32)
    q = fq(v, inv_scale, zero, qbits)
    row = np.repeat(np.arange(n), np.diff(np.asarray(rowptr_norm[:n + 1], np.int64)))
    live = np.zeros(n, np.int64)
    np.add.at(live, row, (q > 0).astype(np.int64))
    dead = live == 0
    return q, dead, np.where(dead[row], v, q).astype(F32)
