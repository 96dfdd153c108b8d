"""tests/_quant_ref.py without a GPU: the sparse restatement of the quantised layer equals the dense oracle
(oracle/quant_oracle.py::layer) -- H bit for bit, D inside the stage-2 bound -- at the shapes of
test_gpu_quant.py::test_quantised_layer_matches_restatement; the comparison the GPU path tests use rejects each way a
store site can get its epilogue wrong; and the operands the GPU tests are built from hold the edges they are built for
(clipped sums on both bounds, moved roundings, stored adjacency entries that quantise to 0, dead rows)."""
import numpy as np
import pytest
import torch

import _quant_ref as Q
from oracle import quant_oracle as QO

N, M, P = 700, 150, 24
ZERO_ROW, EMPTY_ROW = 5, 11


def _case(bits, seed=0, **override):
    """Operands of one layer at (N, M, P): dense X, CSR adjacency without repeated columns (a dense matrix holds none)."""
    from sgracex1_amd import quant
    c = quant.constants(bits, **override)
    rng = np.random.default_rng([seed, bits])
    X = Q.features(N, M, c, seed + bits, dense=True)
    W = Q.weights(M, P, c, seed + bits)
    att = Q.attention(P, c, seed + bits)
    degs = rng.integers(1, 40, N)
    degs[EMPTY_ROW] = 0
    rp, col, val = Q.adjacency(degs, N, c, seed + bits, dead_rows=(ZERO_ROW,))
    dense = np.zeros((N, N), np.float32)
    row = np.repeat(np.arange(N), np.diff(rp))
    dense[row, col] = val
    nz = dense != 0
    rp2 = np.zeros(N + 1, np.int32)
    rp2[1:] = np.cumsum(nz.sum(1))
    col2 = np.nonzero(nz)[1].astype(np.int32)
    return c, X, W, att, (rp2, col2), dense[nz], dense


@pytest.fixture(scope="module")
def cases():
    store = {}

    def get(bits, **override):
        key = (bits, tuple(sorted(override.items())))
        if key not in store:
            store[key] = _case(bits, **override)
        return store[key]
    return get


def _dense_csr(X):
    nz = X != 0
    rp = np.zeros(X.shape[0] + 1, np.int32)
    rp[1:] = np.cumsum(nz.sum(1))
    return rp, np.nonzero(nz)[1].astype(np.int32), X[nz]


@pytest.mark.parametrize("bits", [8, 4, 2, 1])
@pytest.mark.parametrize("gat", [0, 1])
def test_sparse_reference_equals_the_dense_oracle(cases, bits, gat):
    c, X, W, att, adj, a_val, dense = cases(bits)
    want, _e, _p, Wh = QO.layer(torch.as_tensor(dense), torch.as_tensor(X), torch.as_tensor(W),
                                torch.as_tensor(att).reshape(-1, 1), c, relu=1, compute_attention=gat)
    ref = Q.layer(adj, a_val, X, W, att, c, relu=True, gat=gat)
    assert ref["magnitude"] < Q.EXACT_BELOW
    assert np.array_equal(ref["H"], Wh.numpy()), "H differs from the oracle's"
    # the same X stored as CSR goes through the row-block sums: the same bits
    Hs, mag, _f = Q.stage1(_dense_csr(X), W, c)
    assert np.array_equal(Hs, ref["H"]) and mag == ref["magnitude"]
    rows = np.array([0, 7, 699, 14])
    assert np.array_equal(Q.stage1(_dense_csr(X), W, c, rows=rows)[0], ref["H"][rows])
    assert np.array_equal(Q.stage1(X, W, c, rows=rows)[0], ref["H"][rows])
    Q.check_layer(Wh.numpy(), want.numpy(), ref)
    assert np.abs(ref["D"]).max() > 0 and np.isfinite(ref["bound"]).all()


@pytest.mark.parametrize("bits", [8, 4, 2, 1])
def test_operands_hold_their_edges(cases, bits):
    c, X, W, att, adj, a_val, _dense = cases(bits)
    ref = Q.layer(adj, a_val, X, W, att, c, relu=True, gat=1)
    assert Q.can_clip(c, M)
    Q.assert_edges(ref, c, adj=adj, a_val=a_val, clip_terms=M, gat_rows=(ZERO_ROW, EMPTY_ROW))
    # the quantised attention is not all zero (a constant score would hide the softmax)
    assert np.abs(Q.quantise(att, 1, c)[0]).max() > 0
    # a CSR X built by the helper: hot rows of 16 entries and more reach both clip bounds too
    degs = np.random.default_rng(bits).integers(0, 9, 2000)
    degs[::7] = 40
    Xs = Q.features(2000, M, c, 3, degs=degs)
    H, mag, facts = Q.stage1(Xs, W, c)
    assert mag < Q.EXACT_BELOW and Q.can_clip(c, 40)
    Q.assert_edges(dict(H=H, facts=facts), c, clip_terms=40)
    assert not H[degs == 0].any()


MUTANTS = [("no_requant", 0), ("no_requant", 1), ("no_clip", 0), ("scale_before_relu", 0), ("scale_before_relu", 1),
           ("scale_twice", 0), ("scale_twice", 1), ("fill_unscaled", 1)]


@pytest.mark.parametrize("bits", [8, 2])
@pytest.mark.parametrize("kind,gat", MUTANTS)
def test_checker_rejects_a_wrong_epilogue(cases, kind, gat, bits):
    """Each mutant is the reference with one store site's epilogue wrong; the comparison helper must refuse it.
    (deq_o applied before the ReLU shows only under a negative deq_o, which quant.constants() lets a caller set.)"""
    override = dict(deq_o=-0.37) if kind == "scale_before_relu" else {}
    c, X, W, att, adj, a_val, _dense = cases(bits, **override)
    ref = Q.layer(adj, a_val, X, W, att, c, relu=True, gat=gat)
    Q.check_layer(ref["H"], ref["D"].astype(np.float32), ref)                    # the reference itself passes
    bad = Q.layer(adj, a_val, X, W, att, c, relu=True, gat=gat, mutant=kind)
    if kind in ("no_requant", "no_clip"):
        assert ref["facts"]["clip_hi"] > 0 and ref["facts"]["clip_lo"] > 0
        with pytest.raises(AssertionError, match="H:"):
            Q.check_H(bad["H"], ref["H"], ref["magnitude"])
    else:
        assert np.array_equal(bad["H"], ref["H"])
        if kind == "fill_unscaled":
            assert ref["dead"][ZERO_ROW] and ref["dead"][EMPTY_ROW]
        with pytest.raises(AssertionError, match="D:"):
            Q.check_D(bad["D"].astype(np.float32), ref["D"], ref["bound"])


def test_exactness_condition_is_enforced():
    """check_H refuses to call H exact where the operands' code sums can reach 2^24."""
    from sgracex1_amd import quant
    c = quant.constants(8)
    H = np.zeros((2, 2), np.float32)
    Q.check_H(H, H, (1 << 24) - 1)
    with pytest.raises(AssertionError, match="2\\^24"):
        Q.check_H(H, H, 1 << 24)
    # 602 columns of 8-bit codes at the top of both ranges pass it, 128 do not
    X, W = np.full((1, 602), 1.0, np.float32), np.full((602, 1), 1.0, np.float32)
    assert Q.stage1(X, W, c)[1] >= Q.EXACT_BELOW > Q.stage1(X[:, :128], W[:128], c)[1]
