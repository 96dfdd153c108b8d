"""The GAT row-statistics interface without a GPU: include/sgx.h declares the struct and its entry points, the ctypes
binding carries them with the header's argument counts, and the library's switch exists and keeps today's path by default."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgx.h")
ENTRY_POINTS = ["sgx_gat_aggregate_stats", "sgx_layer_forward_stats", "sgx_gat_backward_edges_stats", "sgx_gat_edge_outputs"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(text, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/sgx.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_the_struct_and_the_entry_points():
    text = _header()
    m = re.search(r"typedef\s+struct\s+sgx_gat_stats\s*\{(.*?)\}\s*sgx_gat_stats\s*;", text, flags=re.S)
    assert m, "struct sgx_gat_stats is not declared"
    fields = re.findall(r"float\s*\*\s*(\w+)\s*;", m.group(1))
    assert fields == ["score_row", "score_col", "row_max", "row_sum"]
    for name in ENTRY_POINTS:
        params = _params(text, name)
        assert any("sgx_gat_stats" in p for p in params), name
        assert "stream" in params[-1], name
    bwd = _params(text, "sgx_gat_backward_edges_stats")
    assert any(p == "float dead_weight" for p in bwd) and any(p == "float *S_out" for p in bwd)
    assert not any(re.search(r"\*\s*[ES]$", p) for p in bwd)
    assert not any(re.search(r"\*\s*[ES]$", p) for p in _params(text, "sgx_gat_aggregate_stats"))
    assert re.search(r"#define\s+SGX_VERSION\s+110\b", text)


def test_binding_matches_the_header():
    from sgracex1_amd import _lib
    text = _header()
    assert [n for n, _ in _lib.GatStats._fields_] == ["score_row", "score_col", "row_max", "row_sum"]
    assert ctypes.sizeof(_lib.GatStats) == 4 * ctypes.sizeof(ctypes.c_void_p)
    for name in ENTRY_POINTS:
        assert name in _lib.SYMBOLS
        fn = getattr(_lib.lib, name)
        assert len(fn.argtypes) == len(_params(text, name)), name
        assert fn.restype is ctypes.c_int


def test_argument_errors_need_no_gpu():
    """NULL statistics (or a NULL member) and the unsupported cases are refused before anything is launched."""
    from sgracex1_amd import _lib
    L = _lib.lib
    one = ctypes.c_void_p(256)                          # never dereferenced: the calls return on their argument checks
    empty = _lib.GatStats()
    partial = _lib.GatStats(256, 256, 256, None)
    for st in (None, ctypes.byref(empty), ctypes.byref(partial)):
        assert L.sgx_gat_aggregate_stats(1, 0, 4, 4, 8, 1, 0.2, one, one, one, one, 8, one, one, 8, None, 0, None, one, st,
                                         None) == -1
        assert L.sgx_gat_edge_outputs(1, 4, 4, 1, 0.2, one, one, one, st, 0.0, one, one, None) == -1
        assert L.sgx_gat_backward_edges_stats(1, 4, 4, 8, 1, 0.2, one, one, one, st, 0.0, one, 8, one, 8, None, None, one, one,
                                              None, None) == -1
    full = _lib.GatStats(256, 256, 256, 256)
    assert L.sgx_gat_backward_edges_stats(1, 4, 4, 8, 2, 0.2, one, one, one, ctypes.byref(full), 0.0, one, 8, one, 8, None, None,
                                          one, one, None, None) == -3          # more than one head
    # fill == NULL wants n_nodes 0 (dead rows give 0) or n_cols (the mean of Wh's rows)
    assert L.sgx_gat_aggregate_stats(1, 0, 4, 4, 8, 1, 0.2, one, one, one, one, 8, one, one, 8, None, 3, None, one,
                                     ctypes.byref(full), None) == -2
    d = _lib.LayerDesc()
    d.N_adj = d.M_adj = 4
    d.M_fea = d.P_w = 8
    d.dtype, d.gemm_mode = 1, 1
    assert L.sgx_layer_forward_stats(ctypes.byref(d), ctypes.byref(full), None) == -3          # gat_mode = 0
    d.gat_mode, d.E = 1, 256
    assert L.sgx_layer_forward_stats(ctypes.byref(d), ctypes.byref(full), None) == -3          # E set
    d.E = None
    assert L.sgx_layer_forward_stats(ctypes.byref(d), None, None) == -1
    assert L.sgx_layer_forward_stats(ctypes.byref(d), ctypes.byref(partial), None) == -1


def test_config_switch_defaults_to_the_edge_outputs():
    from sgracex1_amd import config
    assert config.gat_edge_outputs == 1
    assert "gat_edge_outputs" in config.snapshot() and "gat_edge_outputs" in config.describe()


def test_wrappers_refuse_both_side_outputs_at_once():
    import inspect
    from sgracex1_amd import ops, pynq_shim
    for fn in (ops.gat_aggregate, ops.layer_forward):
        assert inspect.signature(fn).parameters["want_row_stats"].default is False
    assert "want_row_stats" in inspect.signature(pynq_shim.Overlay("gnn_all.bit").mmult_top_0.run_layer).parameters
    assert list(inspect.signature(ops.gat_backward_edges_stats).parameters)[:4] == ["adj", "stats", "G", "Wh"]
    assert list(inspect.signature(ops.gat_edge_outputs).parameters) == ["adj", "stats", "alpha", "dead_weight"]
