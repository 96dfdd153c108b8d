"""The float64 restatement of the GAT aggregate (tests/_gat_ref.py) against the CPU oracle and the package's dense twin,
and the evidence that its comparison catches the softmax and mask mistakes the GPU path tests are there for.  No GPU."""
import numpy as np
import pytest
import torch

import _gat_ref as R


def _oracle_heads(oracle, g, heads, relu):
    """oracle.gat_f64 (one head, square table) on every head's slice; rows behind n_rows are appended empty."""
    n_cols, F = g["Wh"].shape
    f = F // heads
    rowptr = np.concatenate([g["rowptr"], np.full(n_cols - g["n_rows"], g["rowptr"][-1])]).astype(np.int32)
    att = g["att"].reshape(heads, 2 * f)
    D, E, S = [], [], []
    for h in range(heads):
        d, e, s = oracle.gat_f64(relu, (rowptr, g["col"].astype(np.int32), g["val"].astype(np.float32)),
                                 np.ascontiguousarray(g["Wh"][:, h * f:(h + 1) * f]).astype(np.float32),
                                 att[h].astype(np.float32), 0.2)
        D.append(d[:g["n_rows"]]), E.append(e), S.append(s)
    sq = (lambda a: a[0]) if heads == 1 else (lambda a: np.stack(a, 1))
    return dict(D=np.concatenate(D, 1), E=sq(E), S=sq(S))


@pytest.mark.parametrize("kind,dt,heads,f_head", [("plain", "f16", 1, 16), ("plain", "f32", 3, 8), ("plain", "f16", 4, 2),
                                                   ("adversarial", "f16", 1, 8), ("adversarial", "f32", 2, 4)])
def test_restatement_matches_the_oracle_per_head(oracle, kind, dt, heads, f_head):
    g = (R.plain_graph(dt, heads, f_head, seed=3) if kind == "plain"
         else R.adversarial_graph(dt, heads, f_head, seed=3, n_filler=300))
    for relu in (0, 1):
        ref = R.forward(g, heads, relu=bool(relu), out="f32")
        got = _oracle_heads(oracle, g, heads, relu)
        R.check_forward(got, ref, g["names"])
        assert np.array_equal(got["E"], ref["E"].astype(np.float32))       # (fp64 scores, rounded once)


def test_restatement_matches_the_dense_twin():
    """config.acc = 0: FPYNQ_GAT's dense emulation (the -9e15 masked softmax over all N columns, fp32) on a square graph
    with rows without entries, rows of masked entries only, and scores hundreds apart."""
    from sgracex1_amd import config, sgrace
    rng = np.random.default_rng(9)
    n, F = 48, 6
    dense = np.zeros((n, n))
    for i in range(n):
        if i in (5, 47):
            continue                                                   # no entries
        cols = rng.choice(n, int(rng.integers(1, 12)), replace=False)
        dense[i, cols] = np.where(rng.random(len(cols)) < 0.25, -0.25, rng.uniform(0.1, 1.0, len(cols)))
    dense[11][dense[11] != 0] = -0.5                                   # stored, all masked
    dense[12, :4] = [0.0, -0.25, 0.7, -0.25]
    Wh = R._round(rng.standard_normal((n, F)) * 0.5, "f32")
    Wh[:, 0] = rng.choice([-3.0, 0.0, 0.5], n)                        # the row's share of the score
    Wh[:, 1] = rng.choice([0.0, 0.0625, 0.15625, -0.25], n)           # the neighbour's
    att = R._round(rng.standard_normal(2 * F) * 0.3, "f32")
    att[[0, 1, F, F + 1]] = [R.SCALE, 0.0, 0.0, R.SCALE]
    sp = torch.tensor(dense).to_sparse_csr()
    g = dict(rowptr=sp.crow_indices().numpy(), col=sp.col_indices().numpy(), val=sp.values().numpy(), Wh=Wh, att=att,
             n_rows=n, n_cols=n)
    ref = R.forward(g, 1, relu=False, dead_rule="mean", out="f32")
    assert ref["dead"][[5, 11, 47]].all() and np.abs(ref["E"]).max() > 500
    old = config.snapshot()
    try:
        config.acc, config.compute_attention, config.float_type, config.fake_quantization = 0, 1, np.float32, 0
        sgrace.init_SGRACE()
        layer = sgrace.GATConv_SGRACE(n, F)
        with torch.no_grad():
            layer.weight.copy_(torch.tensor(Wh, dtype=torch.float32))
            layer.attention.copy_(torch.tensor(att, dtype=torch.float32).reshape(-1, 1))
        coo = torch.tensor(dense, dtype=torch.float32).to_sparse_coo()
        out = layer(1, 1, 0, torch.eye(n), coo.indices(), coo.values(), coo)
    finally:
        config.restore(old)
        sgrace.init_SGRACE()
    R.check("D", out.detach().double().numpy(), ref["D"], ref["bD"], np.arange(n), {})


_ADV = {}


def _adv(dt, heads, f_head):
    key = (dt, heads, f_head)
    if key not in _ADV:
        _ADV[key] = R.adversarial_graph(dt, heads, f_head, seed=1, n_filler=300)
    return _ADV[key]


MUTANTS = ["max_stored", "max_from_zero", "merge_no_rescale", "mask_ne0", "mask_ge0", "mask_ftz"]


@pytest.mark.parametrize("heads,f_head", [(1, 8), (4, 4)])
@pytest.mark.parametrize("kind", MUTANTS)
def test_mutants_fail_on_the_adversarial_graph(kind, heads, f_head):
    """Each deliberately wrong form is rejected by the comparison the GPU path tests apply (fp32 subnormals exist only in
    an fp32 table, so the flushing mask is tried there)."""
    dt = "f32" if kind == "mask_ftz" else "f16"
    g = _adv(dt, heads, f_head)
    ref = R.forward(g, heads, out=dt)
    bad = R.mutant(g, heads, kind, out=dt)
    with pytest.raises(AssertionError):
        R.check_forward(bad, ref, g["names"], parts=("D", "S"))


@pytest.mark.parametrize("heads,f_head", [(1, 16), (3, 8)])
@pytest.mark.parametrize("kind", ["max_stored", "max_from_zero"])
def test_score_mutants_pass_on_order_one_scores(kind, heads, f_head):
    """The two maximum mistakes give the right answer at the scores of order 1 the older GAT tests use: those tests
    cannot see them."""
    g = R.plain_graph("f16", heads, f_head, seed=5)
    ref = R.forward(g, heads, out="f16")
    assert np.abs(ref["E"]).max() < 10
    R.check_forward(R.mutant(g, heads, kind, out="f16"), ref, g["names"], parts=("D", "S"))


def test_adversarial_graph_holds_its_cases():
    """The named rows are what their names say (on the float64 scores)."""
    for dt in ("f16", "f32"):
        g = R.adversarial_graph(dt, 2, 4, seed=0, n_filler=300)
        ref = R.forward(g, 2, out=dt)
        by = {v: k for k, v in g["names"].items()}
        rp, x, live, val = g["rowptr"], ref["E"][:, 0], ref["live"], g["val"]
        ent = lambda name: slice(rp[by[name]], rp[by[name] + 1])
        s = ent("all_live_le_-500")
        assert (x[s][live[s]] <= -500).all()
        assert (x[ent("all_live_ge_100")] >= 100).all()
        s = ent("masked_150_above_last")
        assert x[s][~live[s]].min() >= x[s][live[s]].max() + 150
        s = ent("spread80")
        assert x[s].max() - x[s].min() >= 79
        assert ref["dead"][[by["dead_empty"], by["dead_all_masked"], by["dead_last_row"], by["long_dead"]]].all()
        assert by["dead_last_row"] == g["n_rows"] - 1
        assert not ref["dead"][by["live_f16_subnormal"]] and live[ent("live_f16_subnormal")].sum() == 3
        assert live[ent("live_f32_subnormal")].sum() == (3 if dt == "f32" else 2)
        assert np.signbit(val[ent("mask_minus_zero")]).sum() == 1
        s = ent("long_task_150_below")
        assert x[s][256:].min() >= x[s][:256].max() + 150
        for n in (8, 9, 32, 33, 64, 65, 256, 257):
            assert rp[by[f"deg{n}"] + 1] - rp[by[f"deg{n}"]] == n
        assert np.array_equal(g["protos"][g["proto_id"]], g["Wh"])
