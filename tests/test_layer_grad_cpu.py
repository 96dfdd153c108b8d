"""The dense twin's layer backward (config.acc = 0: FPYNQ_GAT through autograd) against the float64 restatement of
the reference's backward (tests/_layer_grad_ref.py), and the restatement's two forms against each other.  No GPU."""
import numpy as np
import pytest
import torch

import _layer_grad_ref as R


@pytest.mark.parametrize("bits", [None, 8, 4, 2, 1])
@pytest.mark.parametrize("gat", [0, 1])
def test_dense_twin_backward_matches_the_reference(gat, bits):
    """GATConv_SGRACE at config.acc = 0, quantiser off or w_qbits 8/4/2/1: x.grad, weight.grad and attention.grad
    against the restatement, fed the E / S and dead rows of the twin's own forward.  The twin keeps the UNquantised
    adjacency for the backward's P and mask (SG.py:678-680), while its forward decides the dead rows on the quantised
    one."""
    from sgracex1_amd import config, sgrace
    n, m, p = 40, 12, 6
    rowptr, col, val, rows = R.masked_graph(n, 21 + (bits or 0))
    deg = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(n), deg)
    assert deg[rows["empty"]] == 0
    assert deg[rows["non_positive"]] > 0 and not (val[row == rows["non_positive"]] > 0).any()
    assert (val[row == rows["non_positive"]] == 0).any()
    assert deg[rows["tiny"]] > 0 and (val[row == rows["tiny"]] == R.TINY).all()
    assert ((val[row == rows["tiny_entry"]] > R.TINY).any() and (val[row == rows["tiny_entry"]] == R.TINY).any())
    ei = torch.stack([row, col])
    adj = torch.sparse_coo_tensor(ei, val, (n, n))
    g = torch.Generator().manual_seed(5 + gat)
    X = torch.rand((n, m), generator=g) * (torch.rand((n, m), generator=g) < 0.5)
    W = (torch.rand((m, p), generator=g) * 2 - 1) * 0.7
    att = (torch.rand((2 * p, 1), generator=g) * 2 - 1) * 0.7
    G = torch.randn((n, p), generator=g)
    old = config.snapshot()
    try:
        config.acc, config.compute_attention, config.float_type = 0, gat, np.float32
        config.fake_quantization, config.w_qbits = (0, 32) if bits is None else (1, bits)
        sgrace.init_SGRACE()
        layer = sgrace.GATConv_SGRACE(m, p)
        with torch.no_grad():
            layer.weight.copy_(W), layer.attention.copy_(att)
        x = X.clone().requires_grad_(True)
        out = layer(gat, 1, 1, x, ei, val, adj)
        _x, _w, _out, e, P, _adj = out.grad_fn.saved_tensors
        out.backward(G)
        qc = sgrace.quant_constants
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
    # the forward's dead rows (a uniform softmax row) against the ones of the adjacency it masks with
    masked = val if qc is None else sgrace._fq_unsigned(val, qc.a_s, qc.a_z, qc.w_qbits)
    dead = R.dead_rows_of(rowptr, masked)
    want_dead = {rows["empty"], rows["non_positive"]} | (set() if qc is None else {rows["tiny"]})
    assert set(dead.nonzero().reshape(-1).tolist()) == want_dead
    if gat:
        uniform = (P == P[:, :1]).all(1)
        assert torch.equal(uniform, dead) and torch.allclose(P[dead], torch.full_like(P[dead], 1.0 / n))
    E, S = e[row, col], P[row, col]
    got = dict(grad_input=x.grad, grad_weights=layer.weight.grad)
    if gat:
        got["grad_attention"] = layer.attention.grad
    else:
        assert not layer.attention.grad.any()
    grads, bounds = R.dense(rowptr, col, val, X, W, G, gat=bool(gat), E=E, S=S, dead=dead)
    R.check(got, grads, bounds, 1e-5, (gat, bits))


@pytest.mark.parametrize("gat", [0, 1])
def test_reference_dense_and_edge_forms_agree(gat):
    """The N x N form and the edge-list form of the restatement, dead rows included, give the same gradients and the
    same bounds."""
    n, m, p = 300, 20, 9
    g = torch.Generator().manual_seed(7)
    rowptr, col, val, rows = R.masked_graph(n, 3)
    nnz = int(rowptr[-1])
    X = torch.randn((n, m), generator=g, dtype=torch.float64)
    W = torch.randn((m, p), generator=g, dtype=torch.float64)
    G = torch.randn((n, p), generator=g, dtype=torch.float64)
    E = torch.randn(nnz, generator=g, dtype=torch.float64)
    S = torch.rand(nnz, generator=g, dtype=torch.float64)
    dead = R.dead_rows_of(rowptr, val)
    dead[rows["tiny"]] = True                                      # as a quantised forward would decide
    assert int(dead.sum()) == 3
    gd, bd = R.dense(rowptr, col, val, X, W, G, gat=bool(gat), E=E, S=S, dead=dead)
    ge, be = R.edges(rowptr, col, val, X, W, G, gat=bool(gat), E=E, S=S, dead=dead)
    assert set(gd) == set(ge) == set(bd) == set(be) == ({"grad_input", "grad_weights"} | ({"grad_attention"} if gat else set()))
    for k in gd:
        torch.testing.assert_close(ge[k], gd[k], rtol=1e-12, atol=1e-12 * float(bd[k].abs().max()))
        torch.testing.assert_close(be[k], bd[k], rtol=1e-12, atol=0)
