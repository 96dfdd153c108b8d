"""The evaluation head without a GPU: sgx_head_eval is declared, exported and bound with matching argument counts under
the unchanged version, every argument error it documents answers before anything reaches a device, and the numpy
restatement the GPU test trusts (tests/_head_eval_ref.py) agrees with torch's CrossEntropyLoss(reduction="sum") and
argmax on the CPU at the GPU test's shapes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _head_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgx.h")
OK, NULL, SHAPE, UNSUPPORTED, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -7


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared in include/sgx.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_symbols_are_declared_exported_and_bound(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_head_eval_workspace_bytes", "sgx_head_eval"):
        assert name in L.SYMBOLS
        assert re.search(r" T %s\b" % name, out), name
        assert len(getattr(L.lib, name).argtypes) == len(_declaration(name)), name
    assert L.lib.sgx_head_eval.restype is ctypes.c_int
    assert L.lib.sgx_head_eval_workspace_bytes.restype is ctypes.c_size_t


def test_version_is_unchanged(L):
    assert int(re.search(r"#define\s+SGX_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 110
    assert L.lib.sgx_version() == 110


def test_status_codes_are_the_headers(L):
    text = open(HEADER).read()
    for name, code in (("SGX_ERR_NULL", NULL), ("SGX_ERR_SHAPE", SHAPE), ("SGX_ERR_UNSUPPORTED", UNSUPPORTED),
                       ("SGX_ERR_WORKSPACE", WORKSPACE), ("SGX_ERR_ALIGN", ALIGN)):
        assert int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, text).group(1)) == code, name


def test_argument_errors_need_no_gpu(L):
    """Every refusal returns before a launch: the pointers are host addresses that are never dereferenced."""
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p(base)                      # stands for every operand
    ws, wsb = ctypes.c_void_p(base), 4096 + 512

    def call(G=4, n_real=4, P=8, C=2, pooled=p, W=p, bias=p, target=p, totals=p, loss_sum=p, logits=None, ws=ws, wsb=wsb):
        return L.lib.sgx_head_eval(G, n_real, P, C, pooled, W, bias, target, totals, loss_sum, logits, ws, wsb, None)

    need = L.lib.sgx_head_eval_workspace_bytes(4, 8, 2)
    assert need == 256 + 256 + 4096 and need <= wsb
    assert L.lib.sgx_head_eval_workspace_bytes(257, 1, 1) == 256 + 1280 + 4096
    for field in ("pooled", "W", "target", "totals", "loss_sum"):
        assert call(**{field: None}) == NULL, field
    for bad in (dict(n_real=-1), dict(n_real=5), dict(P=0), dict(C=0), dict(G=0, n_real=0)):
        assert call(**bad) == SHAPE, bad
    # the shapes sgx_head_loss refuses
    assert call(P=1025) == UNSUPPORTED and call(C=65) == UNSUPPORTED
    assert L.lib.sgx_head_loss(4, 1025, 2, p, p, p, p, 0.0, 1, 0, None, 1.0, p, None, p, p, p, ws, wsb, None) == UNSUPPORTED
    assert L.lib.sgx_head_eval_workspace_bytes(4, 1025, 2) == 0 and L.lib.sgx_head_eval_workspace_bytes(4, 8, 65) == 0
    assert L.lib.sgx_head_eval_workspace_bytes(0, 8, 2) == 0
    assert call(ws=None) == WORKSPACE and call(wsb=need - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(base + 64)) == ALIGN
    # no real graph and no logits wanted: a valid call that launches nothing
    assert call(n_real=0) == OK


def test_fmaf_restatement_rounds_once():
    """The reference's fmaf against exact rational arithmetic, on operands chosen to sit at rounding ties of the float64
    intermediate as well as on random ones."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, 4000).astype(np.float32)
    b = rng.uniform(-1, 1, 4000).astype(np.float32)
    c = (rng.uniform(-1, 1, 4000) * 2.0 ** rng.integers(-30, 3, 4000)).astype(np.float32)
    a[:4] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(3), np.float32(1 - 2.0 ** -24)
    b[:4] = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -24), np.float32(2.0 ** -25), np.float32(1 - 2.0 ** -24)
    c[:4] = np.float32(2.0 ** -60), np.float32(-2.0 ** -70), np.float32(1), np.float32(2.0 ** -80)
    got = R.fmaf(a, b, c)

    def nearest_f32(q):
        f = np.float32(float(q))                   # a candidate; the exact answer is it or a neighbour
        cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(np.float32(v).view(np.int32)) & 1))
        return np.float32(best)

    for k in range(a.size):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        assert got[k] == nearest_f32(exact), k


@pytest.mark.parametrize("G", R.GRAPHS)
@pytest.mark.parametrize("P", R.WIDTHS)
@pytest.mark.parametrize("C", R.CLASSES)
def test_reference_against_torch(G, P, C):
    case = R.make_case(G, P, C)
    z32 = R.logits_f32(case["pooled"], case["W"], case["bias"])
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    z64 = f64(case["pooled"]) @ f64(case["W"]).T + f64(case["bias"])
    # the fp32 logits lie within the rule's gamma(P + 1) bound of float64's
    e_z = R.gamma(P + 1) * (np.abs(case["pooled"]).astype(np.float64) @ np.abs(case["W"]).astype(np.float64).T
                            + np.abs(case["bias"]).astype(np.float64)) + R.TINY
    assert np.all(np.abs(z32.astype(np.float64) - z64.numpy()) <= e_z)
    # the rule's arg-max is torch's on the same logits
    assert np.array_equal(R.argmax_first(z32), torch.from_numpy(z32).argmax(1).numpy())
    ce = torch.nn.CrossEntropyLoss(reduction="sum")
    for n_real in R.n_reals(G):
        (n, hits), loss, bound = R.eval_ref(case["pooled"], case["W"], case["bias"], case["target"], n_real)
        t = torch.from_numpy(case["target"][:n_real])
        live = (t >= 0) & (t < C)
        assert n == n_real and bound >= 0.0
        assert hits == int((live & (torch.from_numpy(z32[:n_real]).argmax(1) == t)).sum())
        want = float(ce(z64[:n_real][live], t[live])) if bool(live.any()) else 0.0
        assert abs(loss - want) <= 1e-12 * max(1.0, abs(want))
        # the bound is a small multiple of fp32's roundoff per row, not a chosen constant
        assert bound <= R.TINY + n_real * 64 * (P + C + 8) * R.U


def test_tie_case_has_exact_ties():
    case = R.make_tie_case()
    z = R.logits_f32(case["pooled"], case["W"], case["bias"])
    z64 = case["pooled"].astype(np.float64) @ case["W"].astype(np.float64).T + case["bias"]
    assert np.array_equal(z.astype(np.float64), z64)                 # integers: exact in any order
    assert np.array_equal(z[:, 2], z[:, 5]) and np.all(z[:, 2] > np.delete(z, (2, 5), axis=1).max(1))
    G = z.shape[0]
    (n, hits), _, _ = R.eval_ref(case["pooled"], case["W"], case["bias"], case["target"], G)
    assert (n, hits) == (G, (G + 1) // 2)
    assert np.array_equal(R.argmax_first(z), torch.from_numpy(z).argmax(1).numpy())      # torch's tie rule: the first maximum
