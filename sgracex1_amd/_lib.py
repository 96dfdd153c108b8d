"""ctypes binding of libsgx.so (the C ABI declared in include/sgx.h).

The library is the only backend.  If it is missing or does not load, importing this module
raises -- there is no CPU or PyTorch fallback for the accelerated path.
"""
import ctypes
import os

# PyTorch-ROCm ships its own HIP runtime; importing it first makes that copy the one this process
# (and libsgx.so, whose libamdhip64 dependency then resolves to it) uses -- two runtimes in one
# process cannot share streams or allocations.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# SGX_LIB_PATH selects another build of the same library (tools/sweep_spmm.py compares variants)
LIB_PATH = os.environ.get("SGX_LIB_PATH") or os.path.join(_HERE, "csrc", "libsgx.so")

SGX_F16, SGX_F32 = 0, 1
SGX_ACC_F32, SGX_ACC_REF_HALF = 0, 1
SGX_ORDER_REFERENCE, SGX_ORDER_AGGREGATE_FIRST = 0, 1      # sgx_layer_order
SGX_QUANT_INT8 = 2                                          # sgx_quant.flags: integer operands on the int8 matrix cores
SGX_QUANT_INT8_AUTO = 4                                     # ... where they are the faster form (M_fea > 128)
SGX_ERR_SEEDS = -8                                          # sgx_sample_neighbors: a repeated or out-of-range seed
SGX_ERR_BLOCKS = -9                                         # sgx_batch_plan_create: an edge leaves its graph / bad graph_ptr
SGX_BATCH_FORWARD, SGX_BATCH_BACKWARD = 0, 1                # sgx_batch_kind: whose LDS tiles set a batch plan's row budget
SGX_NODE_LOSS_ROWS, SGX_NODE_LOSS_GRID = 16, 512                  # sgx_node_loss: rows of a block, slices at most
SGX_CSR_TRANSPOSE_TILE = 2048                               # sgx_csr_transpose: stored entries per workgroup of a sort pass

# every symbol include/sgx.h declares (tests/test_abi.py checks header and library against this)
SYMBOLS = [
    "sgx_plan_create", "sgx_plan_create_ex", "sgx_plan_destroy", "sgx_plan_long_rows", "sgx_plan_long_threshold", "sgx_plan_natural_utilization",
    "sgx_plan_reordered", "sgx_plan_export", "sgx_xw_sparse_form",
    "sgx_fake_quantize", "sgx_requantize",
    "sgx_layer_workspace_bytes", "sgx_layer_forward",
    "sgx_spmm_csr", "sgx_spmm_csr_acc", "sgx_spmm_scratch_bytes", "sgx_xw_dense", "sgx_xw_sparse", "sgx_transpose",
    "sgx_gat_aggregate", "sgx_gat_scratch_bytes", "sgx_csr_validate", "sgx_coo_to_csr", "sgx_relu_mask_backward",
    "sgx_xt_g", "sgx_xt_g_workspace_bytes", "sgx_readout_mean_linear", "sgx_readout_mean_backward", "sgx_gat_backward_edges",
    "sgx_stream_copy", "sgx_xw_dense_act", "sgx_event_create", "sgx_event_destroy", "sgx_event_record", "sgx_event_elapsed_ms",
    "sgx_gat_aggregate_fill", "sgx_col_sums", "sgx_col_sums_scratch_bytes", "sgx_pack_rows",
    "sgx_code_bias", "sgx_quantize_codes_i8", "sgx_xw_dense_i8", "sgx_xw_dense_i8_workspace_bytes",
    "sgx_sample_workspace_bytes", "sgx_sample_neighbors",
    "sgx_batch_plan_create", "sgx_batch_plan_destroy", "sgx_batch_plan_rows", "sgx_batch_plan_groups",
    "sgx_batch_plan_max_graph", "sgx_batch_plan_fits", "sgx_stack_workspace_bytes", "sgx_stack_forward",
    "sgx_batch_plan_create_ex", "sgx_stack_backward_workspace_bytes", "sgx_stack_backward",
    "sgx_collate_graphs_padded", "sgx_batch_plan_regroup",
    "sgx_collate_graphs", "sgx_collate_graphs_extras", "sgx_batch_plan_group_count", "sgx_batch_plan_create_known", "sgx_batch_plan_export_groups",
    "sgx_gat_aggregate_stats", "sgx_layer_forward_stats", "sgx_gat_edge_outputs", "sgx_gat_backward_edges_stats",
    "sgx_node_batch_workspace_bytes", "sgx_node_batch_sample", "sgx_node_batch_sample_quant",
    "sgx_node_batch_pad_capacity", "sgx_node_batch_sample_padded",
    "sgx_layer_backward_workspace_bytes", "sgx_layer_backward", "sgx_gat_attention_grad_workspace_bytes",
    "sgx_gat_attention_grad",
    "sgx_csr_transpose_workspace_bytes", "sgx_csr_transpose",
    "sgx_gat_stack_workspace_bytes", "sgx_gat_stack_forward",
    "sgx_quant_stack_workspace_bytes", "sgx_quant_stack_forward",
    "sgx_gat_stack_backward_workspace_bytes", "sgx_gat_stack_backward_lds_bytes", "sgx_gat_stack_backward",
    "sgx_quant_stack_backward_workspace_bytes", "sgx_quant_stack_backward_lds_bytes", "sgx_quant_stack_backward",
    "sgx_head_loss_workspace_bytes", "sgx_head_loss", "sgx_adam_step",
    "sgx_node_loss_workspace_bytes", "sgx_node_loss",
    "sgx_head_eval_workspace_bytes", "sgx_head_eval",
    "sgx_version", "sgx_status_string", "sgx_reload_env",
]


class SgxError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        super().__init__(f"{where}: {status_string(status)} (sgx_status {status})")


SGX_QUANT_ADJ_DONE = 1


class Quant(ctypes.Structure):
    """struct sgx_quant -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("qbits", ctypes.c_int32), ("scale_fea", ctypes.c_int32), ("internal_bits", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("inv_scale_fea", ctypes.c_float), ("zero_fea", ctypes.c_float),
        ("inv_scale_w", ctypes.c_float), ("zero_w", ctypes.c_float),
        ("inv_scale_adj", ctypes.c_float), ("zero_adj", ctypes.c_float),
        ("deq_factor", ctypes.c_float), ("reserved", ctypes.c_float),
        ("nnz_adj", ctypes.c_int64), ("nnz_fea", ctypes.c_int64),
    ]


class LayerDesc(ctypes.Structure):
    """struct sgx_layer_desc -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("gemm_mode", ctypes.c_int32), ("relu", ctypes.c_int32), ("gat_mode", ctypes.c_int32),
        ("N_adj", ctypes.c_int32), ("M_adj", ctypes.c_int32), ("M_fea", ctypes.c_int32),
        ("P_w", ctypes.c_int32), ("bias_count", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("acc_mode", ctypes.c_int32), ("spmm_block", ctypes.c_int32), ("gat_fill_dead_rows", ctypes.c_int32),
        ("B", ctypes.c_void_p), ("D", ctypes.c_void_p),
        ("rowPtr_fea", ctypes.c_void_p), ("columnIndex_fea", ctypes.c_void_p), ("values_fea", ctypes.c_void_p),
        ("rowPtr_adj", ctypes.c_void_p), ("columnIndex_adj", ctypes.c_void_p), ("values_adj", ctypes.c_void_p),
        ("attention", ctypes.c_void_p), ("E", ctypes.c_void_p), ("S", ctypes.c_void_p),
        ("alpha", ctypes.c_float), ("fea_threads", ctypes.c_int32), ("adj_threads", ctypes.c_int32),
        ("gat_heads", ctypes.c_int32),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
        ("plan_adj", ctypes.c_void_p), ("plan_fea", ctypes.c_void_p),
        ("ev_agg_begin", ctypes.c_void_p), ("ev_agg_end", ctypes.c_void_p),
        ("quant", ctypes.POINTER(Quant)),
        ("order", ctypes.c_int32),
    ]


class GatStats(ctypes.Structure):
    """struct sgx_gat_stats -- field order and types must match include/sgx.h."""
    _fields_ = [("score_row", ctypes.c_void_p), ("score_col", ctypes.c_void_p), ("row_max", ctypes.c_void_p),
                ("row_sum", ctypes.c_void_p)]


class StackLayer(ctypes.Structure):
    """struct sgx_stack_layer -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("gemm_mode", ctypes.c_int32), ("relu", ctypes.c_int32), ("M_fea", ctypes.c_int32), ("P_w", ctypes.c_int32),
        ("B", ctypes.c_void_p), ("D", ctypes.c_void_p), ("ldd", ctypes.c_int64),
    ]


class StackDesc(ctypes.Structure):
    """struct sgx_stack_desc -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("dtype", ctypes.c_int32), ("n_layers", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_graphs", ctypes.c_int32),
        ("graph_ptr", ctypes.c_void_p),
        ("rowPtr_adj", ctypes.c_void_p), ("columnIndex_adj", ctypes.c_void_p), ("values_adj", ctypes.c_void_p),
        ("rowPtr_fea", ctypes.c_void_p), ("columnIndex_fea", ctypes.c_void_p), ("values_fea", ctypes.c_void_p),
        ("layer", StackLayer * 4),
        ("C", ctypes.c_int32),
        ("W_head", ctypes.c_void_p), ("bias", ctypes.c_void_p),
        ("pooled", ctypes.c_void_p), ("logits", ctypes.c_void_p),
        ("plan", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class GatStackLayer(ctypes.Structure):
    """struct sgx_gat_stack_layer -- field order and types must match include/sgx.h."""
    _fields_ = StackLayer._fields_ + [
        ("gat_mode", ctypes.c_int32), ("attention", ctypes.c_void_p), ("alpha", ctypes.c_float),
    ]


class GatStackDesc(ctypes.Structure):
    """struct sgx_gat_stack_desc -- field order and types must match include/sgx.h."""
    _fields_ = [(n, GatStackLayer * 4 if n == "layer" else t) for n, t in StackDesc._fields_]


class QuantStackLayer(ctypes.Structure):
    """struct sgx_quant_stack_layer -- field order and types must match include/sgx.h."""
    _fields_ = GatStackLayer._fields_ + [("quant", ctypes.POINTER(Quant))]


class QuantStackDesc(ctypes.Structure):
    """struct sgx_quant_stack_desc -- field order and types must match include/sgx.h."""
    _fields_ = [(n, QuantStackLayer * 4 if n == "layer" else t) for n, t in StackDesc._fields_]


class StackGradLayer(ctypes.Structure):
    """struct sgx_stack_grad_layer -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("gemm_mode", ctypes.c_int32), ("relu", ctypes.c_int32), ("M_fea", ctypes.c_int32), ("P_w", ctypes.c_int32),
        ("W", ctypes.c_void_p), ("D", ctypes.c_void_p), ("ldd", ctypes.c_int64),
        ("grad_W", ctypes.c_void_p), ("G", ctypes.c_void_p),
    ]


class StackGradDesc(ctypes.Structure):
    """struct sgx_stack_grad_desc -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("dtype", ctypes.c_int32), ("n_layers", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_graphs", ctypes.c_int32),
        ("graph_ptr", ctypes.c_void_p),
        ("rowPtr_adj", ctypes.c_void_p), ("columnIndex_adj", ctypes.c_void_p), ("values_adj", ctypes.c_void_p),
        ("rowPtr_fea", ctypes.c_void_p), ("columnIndex_fea", ctypes.c_void_p), ("values_fea", ctypes.c_void_p),
        ("layer", StackGradLayer * 4),
        ("grad_pooled", ctypes.c_void_p),
        ("plan", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class GatStackGradLayer(ctypes.Structure):
    """struct sgx_gat_stack_grad_layer -- field order and types must match include/sgx.h."""
    _fields_ = StackGradLayer._fields_ + [
        ("gat_mode", ctypes.c_int32), ("attention", ctypes.c_void_p), ("alpha", ctypes.c_float),
        ("grad_attention", ctypes.c_void_p), ("S", ctypes.c_void_p), ("E", ctypes.c_void_p),
    ]


class GatStackGradDesc(ctypes.Structure):
    """struct sgx_gat_stack_grad_desc -- field order and types must match include/sgx.h."""
    _fields_ = [(n, GatStackGradLayer * 4 if n == "layer" else t) for n, t in StackGradDesc._fields_]


class QuantStackGradLayer(ctypes.Structure):
    """struct sgx_quant_stack_grad_layer -- field order and types must match include/sgx.h."""
    _fields_ = GatStackGradLayer._fields_ + [("quant", ctypes.POINTER(Quant))]


class QuantStackGradDesc(ctypes.Structure):
    """struct sgx_quant_stack_grad_desc -- field order and types must match include/sgx.h."""
    _fields_ = [(n, QuantStackGradLayer * 4 if n == "layer" else t) for n, t in StackGradDesc._fields_] + [
        ("values_adj_q", ctypes.c_void_p)]


class GraphSet(ctypes.Structure):
    """struct sgx_graph_set -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("n_graphs", ctypes.c_int32), ("n_feat", ctypes.c_int32), ("n_edges", ctypes.c_int64),
        ("node_ptr", ctypes.c_void_p), ("edge_ptr", ctypes.c_void_p), ("edge_index", ctypes.c_void_p),
        ("x", ctypes.c_void_p), ("y", ctypes.c_void_p),
        ("rowPtr_adj", ctypes.c_void_p), ("columnIndex_adj", ctypes.c_void_p), ("values_adj", ctypes.c_void_p),
        ("rowPtr_fea", ctypes.c_void_p), ("columnIndex_fea", ctypes.c_void_p), ("values_fea", ctypes.c_void_p),
    ]


class GraphBatch(ctypes.Structure):
    """struct sgx_graph_batch -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("n_graphs", ctypes.c_int32), ("n_rows", ctypes.c_int32),
        ("n_edges", ctypes.c_int64), ("nnz_adj", ctypes.c_int64), ("nnz_fea", ctypes.c_int64),
        ("index", ctypes.c_void_p),
        ("node_off", ctypes.c_void_p), ("edge_off", ctypes.c_void_p), ("adj_off", ctypes.c_void_p), ("fea_off", ctypes.c_void_p),
        ("x", ctypes.c_void_p), ("edge_index", ctypes.c_void_p), ("batch", ctypes.c_void_p), ("y", ctypes.c_void_p),
        ("graph_ptr", ctypes.c_void_p),
        ("rowPtr_adj", ctypes.c_void_p), ("columnIndex_adj", ctypes.c_void_p), ("values_adj", ctypes.c_void_p * 2),
        ("rowPtr_fea", ctypes.c_void_p), ("columnIndex_fea", ctypes.c_void_p), ("values_fea", ctypes.c_void_p * 2),
    ]


SGX_COLLATE_MAX_EXTRAS = 3


class CollateExtra(ctypes.Structure):
    """struct sgx_collate_extra -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("rowPtr", ctypes.c_void_p), ("columnIndex", ctypes.c_void_p), ("values", ctypes.c_void_p), ("dead_row", ctypes.c_void_p),
        ("nnz", ctypes.c_int64), ("entry_off", ctypes.c_void_p),
        ("rowPtr_out", ctypes.c_void_p), ("columnIndex_out", ctypes.c_void_p), ("values_out", ctypes.c_void_p * 2),
        ("dead_row_out", ctypes.c_void_p),
    ]


class CollatePad(ctypes.Structure):
    """struct sgx_collate_pad -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("n_rows", ctypes.c_int32), ("n_graphs", ctypes.c_int32), ("filler_rows", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("n_edges", ctypes.c_int64), ("nnz_adj", ctypes.c_int64), ("nnz_fea", ctypes.c_int64),
        ("nnz_extra", ctypes.c_int64 * SGX_COLLATE_MAX_EXTRAS),
    ]


class NodeBatch(ctypes.Structure):
    """struct sgx_node_batch -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("rowPtr", ctypes.c_void_p), ("columnIndex", ctypes.c_void_p),
        ("n_nodes", ctypes.c_int32), ("batch", ctypes.c_int32), ("n_hops", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("nnz", ctypes.c_int64),
        ("seeds", ctypes.c_void_p), ("fanouts", ctypes.POINTER(ctypes.c_int32)),
        ("seed", ctypes.c_uint64), ("step", ctypes.c_uint64),
        ("node_map", ctypes.c_void_p), ("n_id", ctypes.c_void_p), ("out_rowPtr", ctypes.c_void_p),
        ("out_col", ctypes.c_void_p), ("edge_pos", ctypes.c_void_p),
        ("max_nodes", ctypes.c_int64), ("max_edges", ctypes.c_int64),
        ("hop_nodes", ctypes.POINTER(ctypes.c_int64)), ("hop_edges", ctypes.POINTER(ctypes.c_int64)),
        ("edge_weight", ctypes.c_void_p), ("fill", ctypes.c_float),
        ("rowPtr_norm", ctypes.c_void_p), ("columnIndex_norm", ctypes.c_void_p), ("values_norm", ctypes.c_void_p),
        ("dead_row", ctypes.c_void_p), ("edge_index", ctypes.c_void_p), ("edge_index_agg", ctypes.c_void_p),
        ("rowPtr_x", ctypes.c_void_p), ("columnIndex_x", ctypes.c_void_p), ("values_x", ctypes.c_void_p),
        ("rowPtr_fea", ctypes.c_void_p), ("columnIndex_fea", ctypes.c_void_p), ("values_fea", ctypes.c_void_p),
        ("fea_capacity", ctypes.c_int64),
        ("y", ctypes.c_void_p), ("y_out", ctypes.c_void_p),
        ("mask", ctypes.c_void_p * 3), ("mask_out", ctypes.c_void_p * 3),
        ("nnz_norm", ctypes.c_int64), ("nnz_fea", ctypes.c_int64),
        ("has_dead_rows", ctypes.c_int32), ("max_row", ctypes.c_int32),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class NodeBatchQuant(ctypes.Structure):
    """struct sgx_node_batch_quant -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("n_sets", ctypes.c_int32), ("qbits", ctypes.c_int32),
        ("inv_scale_adj", ctypes.c_float * 2), ("zero_adj", ctypes.c_float * 2),
        ("values_q", ctypes.c_void_p * 2), ("dead_row_q", ctypes.c_void_p * 2), ("values_lean", ctypes.c_void_p * 2),
        ("has_dead_rows_q", ctypes.c_int32 * 2),
    ]


class NodeBatchPad(ctypes.Structure):
    """struct sgx_node_batch_pad -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("n_rows", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("nnz_norm", ctypes.c_int64), ("nnz_fea", ctypes.c_int64), ("n_edges", ctypes.c_int64),
        ("step", ctypes.c_void_p), ("status", ctypes.c_void_p), ("counts", ctypes.c_void_p),
    ]


class LayerGradDesc(ctypes.Structure):
    """struct sgx_layer_grad_desc -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("gat_mode", ctypes.c_int32), ("gemm_mode", ctypes.c_int32), ("N_adj", ctypes.c_int32), ("M_adj", ctypes.c_int32),
        ("M_fea", ctypes.c_int32), ("P_w", ctypes.c_int32), ("dtype_adj", ctypes.c_int32), ("dtype_x", ctypes.c_int32),
        ("gat_heads", ctypes.c_int32), ("alpha", ctypes.c_float), ("nnz_adj", ctypes.c_int64),
        ("rowPtr_adj", ctypes.c_void_p), ("columnIndex_adj", ctypes.c_void_p), ("values_adj", ctypes.c_void_p),
        ("plan_adj", ctypes.c_void_p),
        ("X", ctypes.c_void_p), ("ldx", ctypes.c_int64),
        ("rowPtr_fea", ctypes.c_void_p), ("columnIndex_fea", ctypes.c_void_p), ("values_fea", ctypes.c_void_p),
        ("plan_fea", ctypes.c_void_p),
        ("rowPtr_xt", ctypes.c_void_p), ("columnIndex_xt", ctypes.c_void_p), ("values_xt", ctypes.c_void_p),
        ("plan_xt", ctypes.c_void_p),
        ("W", ctypes.c_void_p), ("G", ctypes.c_void_p), ("ldg", ctypes.c_int64),
        ("E", ctypes.c_void_p), ("S", ctypes.c_void_p), ("stats", ctypes.POINTER(GatStats)), ("dead_weight", ctypes.c_float),
        ("dead", ctypes.c_void_p),
        ("grad_weights", ctypes.c_void_p), ("grad_attention", ctypes.c_void_p), ("grad_input", ctypes.c_void_p),
        ("ld_gi", ctypes.c_int64),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


SGX_ADAM_MAX_TENSORS = 16


class AdamTensor(ctypes.Structure):
    """struct sgx_adam_tensor -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("param", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("grad", ctypes.c_void_p),
        ("n", ctypes.c_int64), ("param_t_out", ctypes.c_void_p),
        ("dtype_t", ctypes.c_int32), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
    ]


class AdamDesc(ctypes.Structure):
    """struct sgx_adam_desc -- field order and types must match include/sgx.h."""
    _fields_ = [
        ("n_tensors", ctypes.c_int32),
        ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
        ("weight_decay", ctypes.c_double),
        ("step", ctypes.c_void_p),
        ("tensor", AdamTensor * SGX_ADAM_MAX_TENSORS),
    ]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP library first (python -m sgracex1_amd.build); "
            "sgracex1_amd has no other backend")
    lib = ctypes.CDLL(LIB_PATH)
    c_int, c_i64, vp, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    lib.sgx_plan_create.argtypes = [ctypes.POINTER(vp), vp, c_int, c_int, vp]
    lib.sgx_plan_create.restype = c_int
    lib.sgx_plan_create_ex.argtypes = [ctypes.POINTER(vp), vp, c_int, c_int, c_int, vp]
    lib.sgx_plan_create_ex.restype = c_int
    lib.sgx_plan_destroy.argtypes = [vp]
    lib.sgx_plan_destroy.restype = None
    lib.sgx_plan_long_rows.argtypes = [vp]
    lib.sgx_plan_long_rows.restype = c_int
    lib.sgx_plan_long_threshold.argtypes = [vp]
    lib.sgx_plan_long_threshold.restype = c_int
    lib.sgx_plan_natural_utilization.argtypes = [vp]
    lib.sgx_plan_natural_utilization.restype = ctypes.c_float
    lib.sgx_plan_reordered.argtypes = [vp]
    lib.sgx_plan_reordered.restype = c_int
    lib.sgx_plan_export.argtypes = [vp, c_int, vp, ctypes.c_int64, vp]
    lib.sgx_plan_export.restype = ctypes.c_int64
    lib.sgx_xw_sparse_form.argtypes = [c_int, c_int, c_int, c_int, vp, c_i64, vp, c_i64, vp]
    lib.sgx_xw_sparse_form.restype = c_int
    lib.sgx_fake_quantize.argtypes = [c_int, c_int, ctypes.c_float, ctypes.c_float, c_i64, vp, vp, vp]
    lib.sgx_fake_quantize.restype = c_int
    lib.sgx_requantize.argtypes = [c_int, c_int, c_i64, vp, c_int, c_int, vp]
    lib.sgx_requantize.restype = c_int
    lib.sgx_layer_workspace_bytes.argtypes = [ctypes.POINTER(LayerDesc)]
    lib.sgx_layer_workspace_bytes.restype = sz
    lib.sgx_layer_forward.argtypes = [ctypes.POINTER(LayerDesc), vp]
    lib.sgx_layer_forward.restype = c_int
    lib.sgx_spmm_csr.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, vp, vp, c_i64, vp, c_i64,
                                 vp, vp, sz, vp]
    lib.sgx_spmm_csr.restype = c_int
    lib.sgx_spmm_csr_acc.argtypes = [c_int, c_int, c_int, c_int, c_int, vp, vp, vp, vp, c_i64, vp, c_i64,
                                     vp, vp, c_i64, vp, vp, sz, vp]
    lib.sgx_spmm_csr_acc.restype = c_int
    lib.sgx_spmm_scratch_bytes.argtypes = [vp, c_int]
    lib.sgx_spmm_scratch_bytes.restype = sz
    lib.sgx_xw_dense.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, vp, c_i64, vp, c_i64, vp, c_i64, vp]
    lib.sgx_xw_dense.restype = c_int
    lib.sgx_xw_sparse.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, vp, vp, c_i64, vp, c_i64,
                                  vp, vp, sz, vp]
    lib.sgx_xw_sparse.restype = c_int
    lib.sgx_transpose.argtypes = [c_int, c_int, c_int, vp, c_i64, vp, c_i64, vp]
    lib.sgx_transpose.restype = c_int
    lib.sgx_gat_scratch_bytes.argtypes = [c_int, c_int, c_int, c_int, vp]
    lib.sgx_gat_scratch_bytes.restype = sz
    lib.sgx_gat_aggregate.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_float, vp, vp, vp, vp, c_i64, vp,
                                      vp, c_i64, vp, vp, vp, vp, vp]
    lib.sgx_gat_aggregate.restype = c_int
    lib.sgx_gat_aggregate_fill.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_float, vp, vp, vp, vp, c_i64, vp,
                                           vp, c_i64, vp, vp, vp, c_i64, vp, vp, vp]
    lib.sgx_gat_aggregate_fill.restype = c_int
    lib.sgx_col_sums_scratch_bytes.argtypes = [c_int]
    lib.sgx_col_sums_scratch_bytes.restype = sz
    lib.sgx_col_sums.argtypes = [c_int, c_int, c_int, vp, c_i64, vp, vp, vp]
    lib.sgx_col_sums.restype = c_int
    lib.sgx_code_bias.argtypes = [c_int, c_int]
    lib.sgx_code_bias.restype = c_int
    lib.sgx_quantize_codes_i8.argtypes = [c_int, c_int, ctypes.c_float, ctypes.c_float, c_int, c_int, vp, c_i64, vp, c_i64, vp]
    lib.sgx_quantize_codes_i8.restype = c_int
    lib.sgx_xw_dense_i8_workspace_bytes.argtypes = [c_int]
    lib.sgx_xw_dense_i8_workspace_bytes.restype = sz
    lib.sgx_xw_dense_i8.argtypes = [c_int, c_int, c_int, c_int, vp, c_i64, vp, c_i64, c_int, c_int, vp, c_i64, vp, vp]
    lib.sgx_xw_dense_i8.restype = c_int
    lib.sgx_pack_rows.argtypes = [c_int, c_i64, c_int, vp, c_i64, vp, vp, c_i64, vp]
    lib.sgx_pack_rows.restype = c_int
    lib.sgx_csr_validate.argtypes = [vp, vp, c_int, c_int, c_i64, vp]
    lib.sgx_csr_validate.restype = c_int
    lib.sgx_coo_to_csr.argtypes = [vp, c_i64, c_int, vp, vp]
    lib.sgx_coo_to_csr.restype = c_int
    lib.sgx_relu_mask_backward.argtypes = [c_int, vp, c_int, vp, c_i64, vp]
    lib.sgx_relu_mask_backward.restype = c_int
    lib.sgx_gat_backward_edges.argtypes = [c_int, c_int, c_int, c_int, ctypes.c_float, vp, vp, vp, vp, vp, vp, c_i64, vp,
                                           c_i64, vp, vp, vp, vp, vp]
    lib.sgx_gat_backward_edges.restype = c_int
    stp = ctypes.POINTER(GatStats)
    lib.sgx_gat_aggregate_stats.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_float, vp, vp, vp, vp, c_i64, vp,
                                            vp, c_i64, vp, c_i64, vp, vp, stp, vp]
    lib.sgx_gat_aggregate_stats.restype = c_int
    lib.sgx_layer_forward_stats.argtypes = [ctypes.POINTER(LayerDesc), stp, vp]
    lib.sgx_layer_forward_stats.restype = c_int
    lib.sgx_gat_edge_outputs.argtypes = [c_int, c_int, c_int, c_int, ctypes.c_float, vp, vp, vp, stp, ctypes.c_float, vp, vp, vp]
    lib.sgx_gat_edge_outputs.restype = c_int
    lib.sgx_gat_backward_edges_stats.argtypes = [c_int, c_int, c_int, c_int, c_int, ctypes.c_float, vp, vp, vp, stp,
                                                 ctypes.c_float, vp, c_i64, vp, c_i64, vp, vp, vp, vp, vp, vp]
    lib.sgx_gat_backward_edges_stats.restype = c_int
    lib.sgx_readout_mean_linear.argtypes = [c_int, c_int, c_int, c_int, vp, c_i64, vp, vp, vp, vp, vp, vp]
    lib.sgx_readout_mean_linear.restype = c_int
    lib.sgx_readout_mean_backward.argtypes = [c_int, c_int, c_int, vp, vp, vp, c_i64, vp]
    lib.sgx_readout_mean_backward.restype = c_int
    lib.sgx_xt_g_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.sgx_xt_g_workspace_bytes.restype = sz
    lib.sgx_xt_g.argtypes = [c_int, c_int, c_int, c_int, vp, c_i64, vp, c_i64, vp, c_i64, vp, sz, vp]
    lib.sgx_xt_g.restype = c_int
    lib.sgx_xw_dense_act.argtypes = [c_int, c_int, c_int, c_int, c_int, vp, c_i64, vp, c_i64, vp, c_i64, vp]
    lib.sgx_xw_dense_act.restype = c_int
    lib.sgx_stream_copy.argtypes = [vp, vp, c_i64, vp]
    lib.sgx_stream_copy.restype = c_int
    lib.sgx_event_create.argtypes = [ctypes.POINTER(vp)]
    lib.sgx_event_create.restype = c_int
    lib.sgx_event_destroy.argtypes = [vp]
    lib.sgx_event_destroy.restype = c_int
    lib.sgx_event_record.argtypes = [vp, vp]
    lib.sgx_event_record.restype = c_int
    lib.sgx_event_elapsed_ms.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float)]
    lib.sgx_event_elapsed_ms.restype = c_int
    i64p, i32p = ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_int32)
    lib.sgx_sample_workspace_bytes.argtypes = [c_int, c_i64, c_int, c_int, i32p, i64p, i64p]
    lib.sgx_sample_workspace_bytes.restype = sz
    lib.sgx_sample_neighbors.argtypes = [vp, vp, c_int, c_i64, vp, c_int, c_int, i32p, ctypes.c_uint64, ctypes.c_uint64,
                                         vp, vp, vp, vp, vp, c_i64, c_i64, i64p, i64p, vp, sz, vp]
    lib.sgx_sample_neighbors.restype = c_int
    lib.sgx_batch_plan_create.argtypes = [c_int, c_int, c_int, vp, vp, vp, c_int, ctypes.POINTER(vp), vp]
    lib.sgx_batch_plan_create.restype = c_int
    lib.sgx_batch_plan_destroy.argtypes = [vp]
    lib.sgx_batch_plan_destroy.restype = c_int
    for name in ("sgx_batch_plan_rows", "sgx_batch_plan_groups", "sgx_batch_plan_max_graph", "sgx_batch_plan_fits"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = c_int
    lib.sgx_stack_workspace_bytes.argtypes = [ctypes.POINTER(StackDesc)]
    lib.sgx_stack_workspace_bytes.restype = sz
    lib.sgx_stack_forward.argtypes = [ctypes.POINTER(StackDesc), vp]
    lib.sgx_stack_forward.restype = c_int
    lib.sgx_batch_plan_create_ex.argtypes = [c_int, c_int, c_int, vp, vp, vp, c_int, c_int, ctypes.POINTER(vp), vp]
    lib.sgx_batch_plan_create_ex.restype = c_int
    lib.sgx_gat_stack_workspace_bytes.argtypes = [ctypes.POINTER(GatStackDesc)]
    lib.sgx_gat_stack_workspace_bytes.restype = sz
    lib.sgx_gat_stack_forward.argtypes = [ctypes.POINTER(GatStackDesc), vp]
    lib.sgx_gat_stack_forward.restype = c_int
    lib.sgx_quant_stack_workspace_bytes.argtypes = [ctypes.POINTER(QuantStackDesc)]
    lib.sgx_quant_stack_workspace_bytes.restype = sz
    lib.sgx_quant_stack_forward.argtypes = [ctypes.POINTER(QuantStackDesc), vp]
    lib.sgx_quant_stack_forward.restype = c_int
    lib.sgx_stack_backward_workspace_bytes.argtypes = [ctypes.POINTER(StackGradDesc)]
    lib.sgx_stack_backward_workspace_bytes.restype = sz
    lib.sgx_stack_backward.argtypes = [ctypes.POINTER(StackGradDesc), vp]
    lib.sgx_stack_backward.restype = c_int
    lib.sgx_gat_stack_backward_workspace_bytes.argtypes = [ctypes.POINTER(GatStackGradDesc)]
    lib.sgx_gat_stack_backward_workspace_bytes.restype = sz
    lib.sgx_gat_stack_backward_lds_bytes.argtypes = [ctypes.POINTER(GatStackGradDesc)]
    lib.sgx_gat_stack_backward_lds_bytes.restype = sz
    lib.sgx_gat_stack_backward.argtypes = [ctypes.POINTER(GatStackGradDesc), vp]
    lib.sgx_gat_stack_backward.restype = c_int
    lib.sgx_quant_stack_backward_workspace_bytes.argtypes = [ctypes.POINTER(QuantStackGradDesc)]
    lib.sgx_quant_stack_backward_workspace_bytes.restype = sz
    lib.sgx_quant_stack_backward_lds_bytes.argtypes = [ctypes.POINTER(QuantStackGradDesc)]
    lib.sgx_quant_stack_backward_lds_bytes.restype = sz
    lib.sgx_quant_stack_backward.argtypes = [ctypes.POINTER(QuantStackGradDesc), vp]
    lib.sgx_quant_stack_backward.restype = c_int
    lib.sgx_collate_graphs.argtypes = [ctypes.POINTER(GraphSet), ctypes.POINTER(GraphBatch), vp]
    lib.sgx_collate_graphs.restype = c_int
    lib.sgx_collate_graphs_extras.argtypes = [ctypes.POINTER(GraphSet), ctypes.POINTER(GraphBatch), ctypes.POINTER(CollateExtra),
                                              c_int, vp]
    lib.sgx_collate_graphs_extras.restype = c_int
    lib.sgx_collate_graphs_padded.argtypes = [ctypes.POINTER(GraphSet), ctypes.POINTER(GraphBatch), ctypes.POINTER(CollateExtra),
                                              c_int, ctypes.POINTER(CollatePad), vp]
    lib.sgx_collate_graphs_padded.restype = c_int
    lib.sgx_batch_plan_regroup.argtypes = [vp, vp, vp]
    lib.sgx_batch_plan_regroup.restype = c_int
    lib.sgx_batch_plan_group_count.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.sgx_batch_plan_group_count.restype = c_int
    lib.sgx_batch_plan_create_known.argtypes = [c_int, c_int, c_int, vp, c_int, c_int, c_int, vp, ctypes.POINTER(vp), vp]
    lib.sgx_batch_plan_create_known.restype = c_int
    lib.sgx_batch_plan_export_groups.argtypes = [vp, vp, c_i64, vp]
    lib.sgx_batch_plan_export_groups.restype = c_i64
    lib.sgx_node_batch_workspace_bytes.argtypes = [c_int, c_i64, c_int, c_int, i32p, i64p, i64p]
    lib.sgx_node_batch_workspace_bytes.restype = sz
    lib.sgx_node_batch_sample.argtypes = [ctypes.POINTER(NodeBatch), vp]
    lib.sgx_node_batch_sample.restype = c_int
    lib.sgx_node_batch_sample_quant.argtypes = [ctypes.POINTER(NodeBatch), ctypes.POINTER(NodeBatchQuant), vp]
    lib.sgx_node_batch_sample_quant.restype = c_int
    lib.sgx_node_batch_pad_capacity.argtypes = [c_int, c_i64, c_int, c_int, i32p, i32p, ctypes.POINTER(NodeBatchPad)]
    lib.sgx_node_batch_pad_capacity.restype = c_int
    lib.sgx_node_batch_sample_padded.argtypes = [ctypes.POINTER(NodeBatch), ctypes.POINTER(NodeBatchPad), vp]
    lib.sgx_node_batch_sample_padded.restype = c_int
    lib.sgx_layer_backward_workspace_bytes.argtypes = [ctypes.POINTER(LayerGradDesc)]
    lib.sgx_layer_backward_workspace_bytes.restype = sz
    lib.sgx_layer_backward.argtypes = [ctypes.POINTER(LayerGradDesc), vp]
    lib.sgx_layer_backward.restype = c_int
    lib.sgx_gat_attention_grad_workspace_bytes.argtypes = [c_int, c_int]
    lib.sgx_gat_attention_grad_workspace_bytes.restype = sz
    lib.sgx_gat_attention_grad.argtypes = [c_int, c_int, c_int, vp, vp, vp, vp, vp, c_i64, vp, vp, sz, vp]
    lib.sgx_gat_attention_grad.restype = c_int
    lib.sgx_csr_transpose_workspace_bytes.argtypes = [c_int, c_int, c_i64]
    lib.sgx_csr_transpose_workspace_bytes.restype = sz
    lib.sgx_csr_transpose.argtypes = [c_int, c_int, c_int, c_i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.sgx_csr_transpose.restype = c_int
    lib.sgx_head_loss_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.sgx_head_loss_workspace_bytes.restype = sz
    lib.sgx_head_loss.argtypes = [c_int, c_int, c_int, vp, vp, vp, vp, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, vp,
                                  ctypes.c_float, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.sgx_head_loss.restype = c_int
    lib.sgx_adam_step.argtypes = [ctypes.POINTER(AdamDesc), vp]
    lib.sgx_adam_step.restype = c_int
    lib.sgx_node_loss_workspace_bytes.argtypes = [c_i64, c_int, c_int]
    lib.sgx_node_loss_workspace_bytes.restype = sz
    lib.sgx_node_loss.argtypes = [c_i64, c_i64, c_int, c_int, vp, vp, vp, vp, vp, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64,
                                  vp, ctypes.c_float, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.sgx_node_loss.restype = c_int
    lib.sgx_head_eval_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.sgx_head_eval_workspace_bytes.restype = sz
    lib.sgx_head_eval.argtypes = [c_int, c_int, c_int, c_int, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.sgx_head_eval.restype = c_int
    lib.sgx_version.argtypes = []
    lib.sgx_version.restype = c_int
    lib.sgx_status_string.argtypes = [c_int]
    lib.sgx_status_string.restype = ctypes.c_char_p
    lib.sgx_reload_env.argtypes = []
    lib.sgx_reload_env.restype = None
    return lib


lib = _load()


def status_string(status):
    return lib.sgx_status_string(int(status)).decode()


def check(status, where):
    if status != 0:
        raise SgxError(status, where)


import contextlib


@contextlib.contextmanager
def tuning(**overrides):
    """Run a block under SGX_* tuning overrides: `with tuning(SGX_XW_NO_WLDS="1"): ...`.  The library reads its
    overrides from the environment once per process (include/sgx.h, sgx_reload_env), so changing os.environ alone does
    nothing after the first call; this sets the variables, has the library read them again, and undoes both on the way
    out.  A value of None removes the variable for the block.  For tests and probes that compare two forms of a kernel."""
    saved = {k: os.environ.get(k) for k in overrides}
    try:
        for k, v in overrides.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        lib.sgx_reload_env()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.sgx_reload_env()
