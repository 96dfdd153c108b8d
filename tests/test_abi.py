"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports exactly what
include/sgx.h declares, the binding _lib derives from the header agrees with the C compiler on every struct,
field and constant and refuses C it does not know, and argument validation answers with the documented
status codes without touching a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgx.h")


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_functions():
    return sorted(set(re.findall(r"\b(sgx_[a-z0-9_]+)\s*\(", _header_text())))


def test_every_declared_symbol_is_exported(L):
    declared = _header_functions()
    assert declared == sorted(L.SYMBOLS) and len(L.SYMBOLS) == len(set(L.SYMBOLS))
    for name in declared:
        assert hasattr(L.lib, name), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (sgx_[a-z0-9_]+)", out))
    assert exported == set(declared)


@pytest.fixture(scope="module")
def compiler_says(L, tmp_path_factory):
    """What the C compiler makes of everything the reader took from the header: {"sizeof T": n, "offsetof T.f": n,
    "fieldsize T.f": n, "const NAME": v}, from one C99 program compiled with -Wall -Werror."""
    body = []
    for c_name, cls in L.ABI.structs.items():
        body.append(f' printf("sizeof {c_name} %zu\\n", sizeof({c_name}));\n')
        for f, _ in cls._fields_:
            body.append(f' printf("offsetof {c_name}.{f} %zu\\n", offsetof({c_name}, {f}));\n')
            body.append(f' printf("fieldsize {c_name}.{f} %zu\\n", sizeof((({c_name} *)0)->{f}));\n')
    for name in L.ABI.constants:
        body.append(f' printf("const {name} %lld\\n", (long long)({name}));\n')
    tmp = tmp_path_factory.mktemp("layout")
    src, exe = tmp / "layout.c", tmp / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n' + "".join(body)
                   + " return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    said = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        kind, what, value = ln.split()
        said[f"{kind} {what}"] = int(value)
    assert len(said) == len(body)
    return said


def test_header_compiles_as_c_and_struct_layout_matches(L, compiler_says):
    """Every struct of the header, not a chosen few: size, the offset of every field, and the size of every field -- a
    4-byte type bound where the header has 8 shows there even when padding hides it from the offsets."""
    declared = re.findall(r"typedef\s+struct\s+(\w+)\s*\{", _header_text())
    assert list(L.ABI.structs) == declared and len(declared) >= 25
    assert {"sgx_layer_desc", "sgx_quant"} <= set(declared)
    for c_name, cls in L.ABI.structs.items():
        assert getattr(L, cls.__name__) is cls and "sgx_" + re.sub(r"(?<!^)([A-Z])", r"_\1", cls.__name__).lower() == c_name
        assert ctypes.sizeof(cls) == compiler_says[f"sizeof {c_name}"], c_name
        for f, ctype in cls._fields_:
            assert getattr(cls, f).offset == compiler_says[f"offsetof {c_name}.{f}"], (c_name, f)
            assert ctypes.sizeof(ctype) == getattr(cls, f).size == compiler_says[f"fieldsize {c_name}.{f}"], (c_name, f)


def test_every_constant_matches_the_compiler(L, compiler_says):
    text = _header_text()
    declared = set(re.findall(r"#define[ \t]+(SGX_\w+)[ \t]+\S", text))
    for body in re.findall(r"typedef\s+enum\s+\w+\s*\{(.*?)\}", text, flags=re.S):
        declared |= set(re.findall(r"(\w+)\s*=", body))
    assert set(L.ABI.constants) == declared and len(declared) >= 27          # 9 #defines, 18 enumerators
    for name, value in L.ABI.constants.items():
        assert compiler_says[f"const {name}"] == value == getattr(L, name), name
    assert (L.SGX_OK, L.SGX_ERR_NULL, L.SGX_ERR_BLOCKS, L.SGX_VERSION, L.SGX_F32, L.SGX_BATCH_BACKWARD) == (0, -1, -9, 110, 1, 1)


def test_representative_signatures(L):
    """One function per kind of type in the header, written out by hand: what the reader must give for them."""
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p as vp

    def sig(name):
        fn = getattr(L.lib, name)
        return fn.restype, list(fn.argtypes)

    assert sig("sgx_spmm_csr") == (c_int, [c_int] * 7 + [vp] * 4 + [c_int64, vp, c_int64, vp, vp, c_size_t, vp])
    assert sig("sgx_head_loss") == (c_int, [c_int] * 3 + [vp] * 4 + [c_float, c_uint64, c_uint64, vp, c_float] + [vp] * 6
                                    + [c_size_t, vp])
    assert sig("sgx_plan_create_ex") == (c_int, [POINTER(vp), vp, c_int, c_int, c_int, vp])
    assert sig("sgx_layer_forward_stats") == (c_int, [POINTER(L.LayerDesc), POINTER(L.GatStats), vp])
    assert sig("sgx_plan_natural_utilization") == (c_float, [vp])
    assert sig("sgx_plan_export") == (c_int64, [vp, c_int, vp, c_int64, vp])
    assert sig("sgx_status_string") == (c_char_p, [c_int])
    assert sig("sgx_reload_env") == (None, [])
    assert sig("sgx_adam_step") == (c_int, [POINTER(L.AdamDesc), vp])
    assert L.AdamTensor._fields_ == [("param", vp), ("m", vp), ("v", vp), ("grad", vp), ("n", c_int64), ("param_t_out", vp),
                                     ("dtype_t", c_int32), ("rows", c_int32), ("cols", c_int32)]
    assert L.AdamDesc._fields_ == [("n_tensors", c_int32), ("lr", c_double), ("beta1", c_double), ("beta2", c_double),
                                   ("eps", c_double), ("weight_decay", c_double), ("step", vp),
                                   ("tensor", L.AdamTensor * 16)]
    # the two kinds of pointer field that are not c_void_p: to a complete struct, and the host arrays of sgx_node_batch
    assert dict(L.LayerDesc._fields_)["quant"] is POINTER(L.Quant)
    assert dict(L.LayerGradDesc._fields_)["stats"] is POINTER(L.GatStats)
    node = dict(L.NodeBatch._fields_)
    assert (node["fanouts"], node["hop_nodes"], node["hop_edges"]) == (POINTER(c_int32), POINTER(c_int64), POINTER(c_int64))
    assert node["seeds"] is vp and node["mask"] is vp * 3 and node["seed"] is c_uint64
    assert dict(L.LayerDesc._fields_)["plan_adj"] is vp and dict(L.NodeBatchQuant._fields_)["values_q"] is vp * 2


_PROLOGUE = "#include <stdint.h>\n#define SGX_N 3\ntypedef struct sgx_ok { int32_t a[SGX_N]; float *p, *q[2]; } sgx_ok;\n"


@pytest.mark.parametrize("bad, line", [
    ("int sgx_f(const sgx_ok *d,\n          int64x_t n);", 5),                          # an unknown type name
    ("typedef struct sgx_s {\n  unsigned flags;\n} sgx_s;", 5),                         # another: no `unsigned` in the ABI
    ("int sgx_f(int n,\n          void (*done)(int), void *stream);", 5),               # a function-pointer parameter
    ("typedef struct sgx_s {\n  int32_t a;\n  int32_t flag : 1;\n} sgx_s;", 6),         # a bit-field
    ("typedef struct sgx_s {\n  float x[SGX_N + 1];\n} sgx_s;", 5),                     # an extent that is an expression
    ("typedef struct sgx_s {\n  float x[SGX_M];\n} sgx_s;", 5),                         # ... or a name never defined
    ("typedef struct sgx_s {\n  float x[2][2];\n} sgx_s;", 5),
    ("typedef struct sgx_s {\n  float **x;\n} sgx_s;", 5),
    ("#define SGX_M (1 << 4)", 4),
    ("typedef enum sgx_e { SGX_A = 0,\n SGX_B } sgx_e;", 5),                             # an enumerator without a value
    ("sgx_ok sgx_f(void);", 4),                                                         # a struct by value
    ("int sgx_f(sgx_ok d);", 4),
    ("int sgx_f(int n, ...);", 4),
])
def test_the_reader_refuses_what_it_does_not_know(bad, line):
    """Strictness: each text is one declaration shape the header does not use.  The reader raises naming the line."""
    from sgracex1_amd import _abi
    good = _abi.read_header(_PROLOGUE)
    assert good.constants == {"SGX_N": 3} and [n for n, _ in good.structs["sgx_ok"]._fields_] == ["a", "p", "q"]
    text = _PROLOGUE + bad + "\n"
    with pytest.raises(_abi.HeaderError) as err:
        _abi.read_header(text, "bad.h")
    assert str(err.value).startswith(f"bad.h:{line}: "), str(err.value)
    assert str(err.value).endswith(text.split("\n")[line - 1].strip()), str(err.value)


def test_version_and_status_strings(L):
    declared = int(re.search(r"#define\s+SGX_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert L.lib.sgx_version() == declared
    assert L.status_string(0) == "ok"
    for code in range(-7, 0):
        assert L.status_string(code) != "unknown status"
    assert L.status_string(-99) == "unknown status"


def test_argument_checks_need_no_gpu(L):
    d = L.LayerDesc()
    assert L.lib.sgx_layer_forward(None, None) == -1                       # SGX_ERR_NULL
    assert L.lib.sgx_layer_workspace_bytes(ctypes.byref(d)) == 0           # M_fea = 0 -> bad desc
    d.N_adj, d.M_adj, d.M_fea, d.P_w = 10, 10, 4, 8
    d.dtype = 7
    assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == -3            # SGX_ERR_UNSUPPORTED
    d.dtype = 0
    d.gemm_mode = 2                                                        # backward-offload mode: not in the public HLS
    assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == -3
    d.gemm_mode = 1
    assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == -1            # buffers missing
    # K.cpp:3876-3889: bias_count > 0 returns before computing anything
    d.bias_count = 3
    assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == 0
    d.bias_count = 0
    need = L.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
    assert need >= 10 * 8 * 2 and need % 256 == 0
    assert L.lib.sgx_spmm_csr(0, 0, 1, 0, 4, 4, 0, None, None, None, None, 8, None, 8, None, None, 0, None) == -2
    assert L.lib.sgx_spmm_csr(0, 0, 1, 0, 4, 4, 8, None, None, None, None, 8, None, 8, None, None, 0, None) == -1
    assert L.lib.sgx_xw_dense(0, 0, 1, 4, 0, 8, None, 8, None, 8, None, 8, None) == -2
    assert L.lib.sgx_transpose(0, 4, 4, None, 4, None, 4, None) == -1
    # aggregate-first order: dense X, GCN aggregate, default arithmetic only; its workspace holds Z = A.X [N_adj][M_fea]
    d.order = 1
    swapped = L.lib.sgx_layer_workspace_bytes(ctypes.byref(d))
    assert 10 * 8 * 2 <= swapped <= need and swapped % 256 == 0
    for field, bad in (("gemm_mode", 0), ("gat_mode", 1), ("acc_mode", 1)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert L.lib.sgx_layer_workspace_bytes(ctypes.byref(d)) == 0, field
        assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == -3, field
        setattr(d, field, keep)
    d.order = 2
    assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == -3
    d.order = 0
    # quantised layer: fp32 only, zero points of the CSR operands must be 0, bit widths bounded
    q = L.Quant()
    q.qbits, q.scale_fea, q.internal_bits = 8, 4, 16
    d.quant = ctypes.pointer(q)
    assert L.lib.sgx_layer_workspace_bytes(ctypes.byref(d)) == 0           # dtype F16 with quant
    d.dtype = 1
    q.nnz_adj = 100
    assert L.lib.sgx_layer_workspace_bytes(ctypes.byref(d)) >= need + 8 * 4 * 4 + 10 * 4 * 4 + 400
    q.zero_adj = 1.0
    assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == -3
    q.zero_adj, q.qbits = 0.0, 40
    assert L.lib.sgx_layer_forward(ctypes.byref(d), None) == -3
    assert L.lib.sgx_fake_quantize(1, 8, 1.0, 0.0, -1, None, None, None) == -2
    assert L.lib.sgx_fake_quantize(1, 0, 1.0, 0.0, 4, None, None, None) == -3
    assert L.lib.sgx_fake_quantize(1, 8, 1.0, 0.0, 4, None, None, None) == -1
    assert L.lib.sgx_requantize(4, 8, 4, None, 4, 16, None) == -2


def test_product_path_has_no_oracle_or_cpu_fallback():
    """Nothing under sgracex1_amd/ may import or link the oracle."""
    pkg = os.path.join(ROOT, "sgracex1_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in text.lower(), (fn, "mentions the oracle")
                assert "liborc" not in text
    # examples/ and tools/ neither: the only importers outside tests/ are bench.py's cpu_baseline leg and
    # __graft_entry__ (build of the checker, smoke's check)
    for sub in ("examples", "tools"):
        for fn in os.listdir(os.path.join(ROOT, sub)):
            if fn.endswith((".py", ".cpp", ".sh")):
                text = open(os.path.join(ROOT, sub, fn)).read()
                assert "from oracle" not in text and "import oracle" not in text and "oracle/" not in text, fn


def test_graft_entry_build_check_passes():
    """`__graft_entry__.build()` is the driver's does-it-build step: run it (the objects are already
    compiled, so this relinks and re-checks) -- a stale version assert there once went unnoticed."""
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    entry = importlib.import_module("__graft_entry__")
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "def build()" in src and "def smoke()" in src
    # everything build() asserts after compiling, without forcing a full recompile here
    from sgracex1_amd import _lib
    declared = int(re.search(r"#define\s+SGX_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert _lib.lib.sgx_version() == declared
    assert callable(entry.build) and callable(entry.smoke)


def test_package_fails_loudly_without_the_library(tmp_path):
    """No HIP library -> importing the accelerated path raises; there is no CPU or torch fallback."""
    import sys
    env = dict(os.environ, SGX_LIB_PATH=str(tmp_path / "no_such_libsgx.so"))
    out = subprocess.run([sys.executable, "-c", "import sgracex1_amd.ops"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode != 0
    assert "ImportError" in out.stderr and "no other backend" in out.stderr
    # a file that is not a loadable library fails too (OSError from the loader), it is not skipped
    bogus = tmp_path / "libsgx.so"
    bogus.write_bytes(b"not an ELF file")
    out = subprocess.run([sys.executable, "-c", "import sgracex1_amd.ops"], cwd=ROOT, env=dict(env, SGX_LIB_PATH=str(bogus)),
                         capture_output=True, text=True)
    assert out.returncode != 0 and "Error" in out.stderr


def test_integration_md_stub_matches_the_header(L):
    """The ctypes stub printed in INTEGRATION.md is field for field the struct of include/sgx.h."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index("class sgx_layer_desc(ctypes.Structure)"):]
    block = block[:block.index("\n\nsgx.sgx_layer_workspace_bytes")]
    scope = {"ctypes": ctypes}
    exec(block, scope)                                                 # defines sgx_layer_desc from the document
    doc = scope["sgx_layer_desc"]
    assert ctypes.sizeof(doc) == ctypes.sizeof(L.LayerDesc)
    assert [n for n, _ in doc._fields_] == [n for n, _ in L.LayerDesc._fields_]
    for name, _ in doc._fields_:
        assert getattr(doc, name).offset == getattr(L.LayerDesc, name).offset, name
