"""Restatement in numpy of the wide form of the sampler's subset step (csrc/sample.hip, sample_wide_kernel): Floyd's loop
of include/sgx.h without the wait of every element for the one before it, in the order the kernel works in -- chunks of
64 elements, the chain words updated in place chunk by chunk.  tests/test_sampler_wide_cpu.py pins it to
_sampler_ref.floyd.

With base = deg - k, j_i = base + i, t_i = draw(j_i):
    dup_i  = t_i is among t_0 .. t_{i-1}
    par_i  = t_i - base where 0 <= t_i - base < i, else none        (j_par is the only j that t_i can equal)
    hit_i  = dup_i or hit[par_i]
    elem_i = j_i if hit_i else t_i
An earlier element equals t_i either as its own draw -- then dup_i, whether that element kept its draw or not, since an
element that did not keep it found it in the set already -- or as its j, which it holds exactly when it was hit.  par_i <
i, so hit is the OR of dup along a chain of falling indices, and ceil(log2 k) rounds of pointer jumping give it."""
import numpy as np

import _sampler_ref as R

LANES = 64


def rounds_of(k):
    """ceil(log2 k) for k >= 2, as 32 - clz(k - 1)."""
    return int(k - 1).bit_length()


def chain_words(t, base):
    """-> dup (bool [k]) and par (int64 [k], -1 = none) before any jumping."""
    k = len(t)
    i = np.arange(k)
    order = np.argsort(t, kind="stable")                   # equal draws side by side, in index order
    dup = np.zeros(k, bool)
    dup[order[1:]] = t[order[1:]] == t[order[:-1]]
    par = t - base
    return dup, np.where((par >= 0) & (par < i), par, -1)


def chain_length(par):
    """The longest chain, counted in elements (an element without a parent is a chain of 1)."""
    depth = np.ones(len(par), np.int64)
    for i in range(len(par)):                              # parents lie below their children
        if par[i] >= 0:
            depth[i] = depth[par[i]] + 1
    return int(depth.max())


def jump(dup, par):
    """hit after rounds_of(k) rounds, every round the chunks in order, a chunk read whole and then written in place."""
    hit, par = dup.copy(), par.copy()
    k = len(hit)
    for _ in range(rounds_of(k)):
        for c0 in range(0, k, LANES):
            s = slice(c0, min(c0 + LANES, k))
            p = par[s]
            has = p >= 0
            q = np.where(has, p, 0)
            new_hit = hit[s] | (has & hit[q])
            new_par = np.where(has, par[q], -1)
            hit[s], par[s] = new_hit, new_par
    return hit, par


def wide(key, v, deg, k):
    """Positions (ascending) sampled from a row of `deg` > k entries, 2 <= k."""
    t = R.draws(key, v, deg, k)
    base = deg - k
    dup, par = chain_words(t, base)
    hit, left = jump(dup, par)
    assert (left < 0).all()                                # every chain was walked to its root
    elem = np.where(hit, base + np.arange(k), t)
    rank = (elem[None, :] < elem[:, None]).sum(1)          # the kernel's slot of every element
    out = np.empty(k, np.int64)
    out[rank] = elem
    return out.tolist()
