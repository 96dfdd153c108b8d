"""The rule of the padded batches that carry the quantised adjacencies (include/sgx.h, "padded batches ready for the
QUANTISED layers") restated in numpy: tests/_padded_ref.padded extended with the quantised value arrays.  A quantised
adjacency shares the normalised adjacency's pattern; behind its live entries the P filler rows' diagonal entries hold the
image of 1 on its unsigned grid and the spare entries up to the capacity the image of 0, both from tests/_quant_ref's
unsigned quantiser (the oracle's quantization_ufbits); the filler rows' bytes are 0.
"""
import numpy as np

import _padded_ref as R
import _quant_ref as Q


def key(c):
    """What ops files a quantised adjacency under: the constants its quantiser reads."""
    return (c.w_qbits, c.a_s, c.a_z)


def fq(x, c):
    """The float32 image of the number x on the unsigned adjacency grid of the constants c."""
    return Q.quantise_adj(np.array([x], np.float32), c)[0]


def inert(c):
    """The call's two preconditions on the adjacency grid of c: the filler rows' 1 stays positive, their spare 0 stays 0."""
    return bool(fq(1.0, c) > 0) and bool(fq(0.0, c) == 0)


def padded(live, cap, n_feat, qcs=()):
    """R.padded(live, cap, n_feat) plus, for every constant set of qcs, q_val[key] / q_dead[key] of the padded batch from
    live["q_val"][key] (float32 [a], over norm_col's pattern) and live["q_dead"][key] (bool [n])."""
    out = R.padded(live, cap, n_feat)
    n, N = live["x"].shape[0], cap["n_rows"]
    a, P = len(live["norm_col"]), N - n
    assert a + P <= cap["nnz_norm"]
    out["q_val"], out["q_dead"] = {}, {}
    for c in qcs:
        k = key(c)
        v = np.full(cap["nnz_norm"], fq(0.0, c), np.float32)
        v[:a], v[a:a + P] = live["q_val"][k], fq(1.0, c)
        out["q_val"][k] = v
        out["q_dead"][k] = np.concatenate([live["q_dead"][k], np.zeros(P, bool)])
    return out
