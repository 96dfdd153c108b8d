"""sgx_head_eval on the device (include/sgx.h, "the evaluation head") against tests/_head_eval_ref.py: exact totals, logits
bit-equal to sgx_head_loss's at p = 0, the summed loss within the bound the reference derives, exact ties, NaN filler
rows that reach no sum, accumulation across calls, and the same bits on every run."""
import numpy as np
import pytest
import torch

import _head_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _dev(case, n_real=None):
    """The case's operands on the device; the filler rows behind n_real hold NaN and a label outside every class range."""
    pooled, target = case["pooled"].copy(), case["target"].copy()
    if n_real is not None:
        pooled[n_real:] = np.nan
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(pooled), t(case["W"]), t(case["bias"]), t(target)


@pytest.mark.parametrize("G", R.GRAPHS)
@pytest.mark.parametrize("P", R.WIDTHS)
@pytest.mark.parametrize("C", R.CLASSES)
def test_totals_logits_and_loss(G, P, C):
    from sgracex1_amd import ops
    case = R.make_case(G, P, C)
    full = _dev(case)
    want_logits = ops.head_loss(*full, p=0.0, want_logits=True)[-1]
    for n_real in R.n_reals(G):
        pooled, W, b, t = _dev(case, n_real)
        totals, loss_sum, logits = ops.head_eval(pooled, W, b, t, n_real=n_real, want_logits=True)
        (n, hits), loss, bound = R.eval_ref(case["pooled"], case["W"], case["bias"], case["target"], n_real)
        got_loss = float(loss_sum.cpu()[0])
        print(f"G={G} P={P} C={C} n_real={n_real}: totals {totals.tolist()} want {[n, hits]}; loss_sum {got_loss!r} "
              f"want {loss!r} error {abs(got_loss - loss):.3e} bound {bound:.3e}")
        assert totals.tolist() == [n, hits]
        assert logits.shape == (G, C) and same_bits(logits[:n_real], want_logits[:n_real])
        assert bool(torch.isnan(logits[n_real:]).all())                  # every row is written; the fillers' are NaN
        assert np.isfinite(got_loss) and abs(got_loss - loss) <= bound
        # without the logits output the filler rows are not read at all: the same sums
        totals2, loss2 = ops.head_eval(pooled, W, b, t, n_real=n_real)
        assert torch.equal(totals2, totals) and same_bits(loss2, loss_sum)


def test_ties_go_to_the_first_maximum():
    from sgracex1_amd import ops
    case = R.make_tie_case()
    G = case["pooled"].shape[0]
    pooled, W, b, t = _dev(case)
    totals, loss_sum, logits = ops.head_eval(pooled, W, b, t, want_logits=True)
    z = logits.cpu().numpy()
    assert np.array_equal(z[:, 2], z[:, 5]) and np.array_equal(z, R.logits_f32(case["pooled"], case["W"], case["bias"]))
    assert totals.tolist() == [G, (G + 1) // 2]
    # every row's loss is log 2 up to the rounding of exp, log and the sum: the reference's bound holds here too
    _, loss, bound = R.eval_ref(case["pooled"], case["W"], case["bias"], case["target"], G)
    assert abs(float(loss_sum.cpu()[0]) - loss) <= bound


@pytest.mark.parametrize("G,P,C", [(65, 65, 7), (257, 64, 2)])
def test_two_calls_accumulate(G, P, C):
    """Two calls into the same accumulators: totals of the concatenation, loss_sum the double sum of the two calls' own."""
    from sgracex1_amd import ops
    a, b2 = R.make_case(G, P, C, seed=1), R.make_case(G - 2, P, C, seed=2)
    b2["W"], b2["bias"] = a["W"], a["bias"]
    n_a, n_b = G - 1, G - 3                                              # padded batches: one filler row each
    A, B = _dev(a, n_a), _dev(b2, n_b)
    ta, la = ops.head_eval(*A, n_real=n_a)
    tb, lb = ops.head_eval(*B, n_real=n_b)
    totals, loss_sum = ops.head_eval(*A, n_real=n_a)
    out = ops.head_eval(*B, n_real=n_b, totals=totals, loss_sum=loss_sum)
    assert out[0] is totals and out[1] is loss_sum
    assert totals.tolist() == (ta + tb).tolist()
    assert float(loss_sum.cpu()[0]) == float(la.cpu()[0]) + float(lb.cpu()[0])       # one double addition
    cat = dict(pooled=np.concatenate([a["pooled"][:n_a], b2["pooled"][:n_b]]), W=a["W"], bias=a["bias"],
               target=np.concatenate([a["target"][:n_a], b2["target"][:n_b]]))
    one, _ = ops.head_eval(*_dev(cat))
    assert one.tolist() == totals.tolist()
    (n, hits), _, _ = R.eval_ref(cat["pooled"], cat["W"], cat["bias"], cat["target"], n_a + n_b)
    assert totals.tolist() == [n, hits]


def test_two_runs_give_the_same_bits():
    from sgracex1_amd import ops
    case = R.make_case(257, 65, 7, seed=3)
    ops_in = _dev(case, 256)
    first = ops.head_eval(*ops_in, n_real=256, want_logits=True)
    torch.cuda.synchronize()
    junk = torch.full((1 << 22,), 0xFF, dtype=torch.uint8, device=DEV)  # the workspace is reused: its old contents must not matter
    del junk
    second = ops.head_eval(*ops_in, n_real=256, want_logits=True)
    for x, y in zip(first, second):
        assert same_bits(x[:256] if x.dim() == 2 else x, y[:256] if y.dim() == 2 else y)


def test_operand_checks():
    from sgracex1_amd import ops
    pooled, W, b, t = _dev(R.make_case(4, 8, 2))
    with pytest.raises(ValueError):
        ops.head_eval(pooled, W, b, t, n_real=5)
    with pytest.raises(TypeError):
        ops.head_eval(pooled, W, b, t, totals=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        ops.head_eval(pooled, W, b, t.int())
