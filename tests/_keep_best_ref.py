"""sgx_keep_best restated in numpy (include/sgx.h, "model selection"): the decision, the state transition, the log row and
the copy, on host arrays.  Everything is int64 / uint32 words; nothing is divided and nothing is a float."""
import numpy as np

FRESH = (1, 0, -1, 0)                     # best_n, best_hits, best_epoch, epoch
LIMIT = 1 << 31

# the hand sequence of the issue as (n, hits): 0/5, 1/3, 2/6, 2/5, 2/5, 1/2, n = 0, hits > n, n = 2^31
SEQUENCE = [(5, 0), (3, 1), (6, 2), (5, 2), (5, 2), (2, 1), (0, 0), (3, 4), (LIMIT, LIMIT)]
BEST_AFTER = [-1, 1, 1, 3, 3, 5, 5, 5, 5]          # best_epoch after each call, worked out by hand


def fresh_state():
    return np.array(FRESH, dtype=np.int64)


def better(n, hits, best_n, best_hits):
    n, hits, best_n, best_hits = int(n), int(hits), int(best_n), int(best_hits)
    if not (0 < n < LIMIT and 0 <= hits <= n and best_n < LIMIT):
        return False
    lhs, rhs = hits * best_n, best_hits * n         # python integers; the bounds keep both inside int64 on a kept state
    return lhs > rhs


def keep_best(srcs, dsts, sums, state, log=None):
    """One call, in place on numpy arrays: srcs / dsts lists of uint32 (or float32) arrays of equal sizes, sums a list of
    int64 [3] arrays, state int64 [4], log int64 [rows, 3 * len(sums)] or None.  Returns whether the epoch won."""
    n, hits, e = int(sums[0][0]), int(sums[0][1]), int(state[3])
    won = better(n, hits, state[0], state[1])
    if log is not None and 0 <= e < log.shape[0]:
        log[e] = np.concatenate([np.asarray(s, dtype=np.int64) for s in sums])
    if won:
        for s, d in zip(srcs, dsts):
            d.view(np.uint32)[...] = s.view(np.uint32)
        state[0], state[1], state[2] = n, hits, e
    state[3] = e + 1
    return won
