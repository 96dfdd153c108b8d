"""Torch-facing wrappers over the C ABI (include/sgx.h).

PyTorch is plumbing here: it owns device memory and the stream.  Every function passes raw
device pointers to libsgx.so and returns torch tensors that alias buffers the call filled.
All tensors must live on a ROCm device ("cuda"); nothing in this module computes on the CPU.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import (SGX_ACC_F32, SGX_ACC_REF_HALF, SGX_F16, SGX_F32, SGX_ORDER_AGGREGATE_FIRST, SGX_ORDER_REFERENCE,
                   LayerDesc, check, lib)

_DTYPES = {torch.float16: SGX_F16, torch.float32: SGX_F32}


def dtype_code(dtype):
    try:
        return _DTYPES[dtype]
    except KeyError:
        raise TypeError(f"sgx supports float16 and float32 element types, got {dtype}") from None


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU (got {type(t).__name__}"
                         f"{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _dev2d(t, name):
    """2-D tensor whose rows may be padded (row stride >= width, unit column stride)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU")
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name} must be 2-D with unit column stride")
    return t


def _out(out, rows, cols, dtype, device, name="out"):
    """A caller-provided result buffer: [rows, >= cols] of the right element type on the right device, unit
    column stride (rows may be padded).  The library writes through the raw pointer, so a wrong buffer must
    be refused here."""
    if out is None:
        return torch.empty((rows, cols), dtype=dtype, device=device)
    _dev2d(out, name)
    if out.dtype != dtype or out.device != device or out.shape[0] != rows or out.shape[1] != cols:
        raise ValueError(f"{name} must be a [{rows}, {cols}] {dtype} tensor on {device} "
                         f"(got {tuple(out.shape)} {out.dtype} on {out.device})")
    return out


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def cached_on(tensor, key, build):
    """Derived data (a CSR, a transposed pattern ...) kept ON the tensor object it was built from, so that it
    lives exactly as long as that tensor and can never be handed to another tensor that happens to reuse the
    address; an in-place change of the tensor (its version counter) rebuilds it."""
    store = tensor.__dict__.setdefault("_sgx_cache", {})
    hit = store.get(key)
    if hit is None or hit[0] != tensor._version:
        hit = store[key] = (tensor._version, build())
    return hit[1]


def attach(tensor, key, value):
    """Fill the cached_on entry `key` of `tensor` with a value built elsewhere (the graph loader hands its batches over with
    their CSRs and graph_ptr already in place); it holds while the tensor is unchanged, as a built entry does."""
    tensor.__dict__.setdefault("_sgx_cache", {})[key] = (tensor._version, value)
    return value


def recorded(tensor, key):
    """The cached_on entry `key` of `tensor` if there is one and the tensor is unchanged since; None otherwise (builds
    nothing)."""
    hit = tensor.__dict__.get("_sgx_cache", {}).get(key)
    return hit[1] if hit is not None and hit[0] == tensor._version else None


_workspaces = {}


def _workspace(device, nbytes):
    """Grow-only scratch per (device, stream); the library itself never allocates."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


class GatStats:
    """The row softmax statistics of a GAT aggregate (struct sgx_gat_stats, include/sgx.h), fp32 on the device:
    score_row [n_rows, heads] = Wh_i . a1, score_col [n_cols, heads] = Wh_c . a2, row_max / row_sum [n_rows, heads] = the
    maximum m_i of a row's live scores and the sum of exp(E_e - m_i) over them (both 0 for a row without a live entry).
    They stand for the per-edge outputs: E_e = LeakyReLU(score_row[i] + score_col[c]), S_e = exp(E_e - m_i) / l_i on a
    live entry, 0 on a masked one (gat_edge_outputs forms them) -- 3 n_rows + n_cols floats per head in place of 2 nnz."""

    def __init__(self, n_rows, n_cols, heads, device):
        self.heads = int(heads)
        shape = (lambda n: (n,)) if self.heads == 1 else (lambda n: (n, self.heads))
        self.score_row = torch.empty(shape(n_rows), dtype=torch.float32, device=device)
        self.score_col = torch.empty(shape(n_cols), dtype=torch.float32, device=device)
        self.row_max = torch.empty(shape(n_rows), dtype=torch.float32, device=device)
        self.row_sum = torch.empty(shape(n_rows), dtype=torch.float32, device=device)

    def tensors(self):
        return self.score_row, self.score_col, self.row_max, self.row_sum

    @classmethod
    def of(cls, score_row, score_col, row_max, row_sum):
        """The statistics over four tensors that exist already (an autograd function's saved tensors)."""
        st = cls.__new__(cls)
        st.heads = 1 if score_row.dim() == 1 else int(score_row.shape[1])
        st.score_row, st.score_col, st.row_max, st.row_sum = score_row, score_col, row_max, row_sum
        return st

    def struct(self):
        for name, t in zip(("score_row", "score_col", "row_max", "row_sum"), self.tensors()):
            _dev(t, name)
            if t.dtype != torch.float32:
                raise TypeError("the GAT statistics are float32 tensors")
        return _lib.GatStats(*(t.data_ptr() for t in self.tensors()))


class Plan:
    """Row schedule of one CSR matrix (sgx_plan): which rows are split across wavefronts."""

    def __init__(self, rowptr, long_threshold=0, chunk=0):
        _dev(rowptr, "rowptr")
        h = ctypes.c_void_p()
        check(lib.sgx_plan_create_ex(ctypes.byref(h), _ptr(rowptr), rowptr.numel() - 1, int(long_threshold), int(chunk),
                                     _stream()), "sgx_plan_create_ex")
        self._h = h
        self.n_rows = rowptr.numel() - 1

    @property
    def handle(self):
        return self._h

    @property
    def long_rows(self):
        return lib.sgx_plan_long_rows(self._h)

    @property
    def long_threshold(self):
        return lib.sgx_plan_long_threshold(self._h)

    @property
    def natural_utilization(self):
        return lib.sgx_plan_natural_utilization(self._h)

    @property
    def reordered(self):
        return bool(lib.sgx_plan_reordered(self._h))

    ARRAYS = ("long_row", "long_first", "task_row", "task_e0", "task_e1", "row_order", "win_order", "scan_win")

    def export(self, name):
        """One of the schedule's device arrays (ARRAYS) as an int32 tensor -- for inspection and tests."""
        which = self.ARRAYS.index(name)
        n = lib.sgx_plan_export(self._h, which, None, 0, _stream())
        if n < 0:
            check(int(n), "sgx_plan_export")
        out = torch.empty(int(n), dtype=torch.int32, device="cuda")
        if n:
            got = lib.sgx_plan_export(self._h, which, _ptr(out), int(n), _stream())
            if got < 0:
                check(int(got), "sgx_plan_export")
        if name == "win_order":                 # bytes: the row (0..63) of every rank of every 64-row window
            return out.view(torch.uint8)
        return out

    def __del__(self, _destroy=lib.sgx_plan_destroy):        # bound at definition: module globals are gone at shutdown
        h, self._h = getattr(self, "_h", None), None
        if h:
            _destroy(h)


class Csr:
    """CSR matrix in HBM: rowptr[int32, n_rows+1], col[int32, nnz], val[f16|f32, nnz]."""

    def __init__(self, rowptr, col, val, n_cols, plan=None):
        self.rowptr = _dev(rowptr, "rowptr")
        self.col = _dev(col, "col")
        self.val = _dev(val, "val")
        if rowptr.dtype != torch.int32 or col.dtype != torch.int32:
            raise TypeError("CSR indices must be int32 (the reference's `int` ports, K.cpp:3769-3773)")
        self.n_rows = rowptr.numel() - 1
        self.n_cols = int(n_cols)
        self._nnz = col.numel()
        if self._nnz == 0:
            # an empty tensor has no address; the library wants non-NULL index / value arrays even when
            # rowPtr says there is nothing to read
            self.col = torch.zeros(1, dtype=torch.int32, device=self.rowptr.device)
            self.val = torch.zeros(1, dtype=val.dtype, device=self.rowptr.device)
        self._plan = plan
        self._dead_rows = None
        self._dead_row_mask = None
        self._dead_rows_version = self._dead_row_mask_version = None      # the values' version a computed answer holds for
        self._max_row = None                   # the longest row, or a bound on it, where the builder knows it
        self._flat = False                     # aggregates by the entry-split form (with_facts(flat=True)): never wants a plan
        self._flat_quant = False               # ... under a quantiser too (with_facts(flat_quant=True)); read only with _flat
        self._quantized = {}

    @property
    def dead_rows(self):
        """bool [n_rows] on the device: the rows that hold no positive value, which the GAT mask `adj > 0` (SG.py:640)
        leaves without a neighbour.  Built once per matrix and state of the values (the value tensor's version counter: an
        in-place change builds it again), without a sync.  A mask given through with_facts stays as given."""
        if self._dead_row_mask is None or self._dead_row_mask_version not in (None, self.val._version):
            deg = (self.rowptr[1:] - self.rowptr[:-1]).long()
            row = torch.repeat_interleave(torch.arange(self.n_rows, device=self.val.device), deg, output_size=self.nnz)
            live = torch.zeros(self.n_rows, dtype=torch.int32, device=self.val.device)
            live.index_add_(0, row, (self.val[:self.nnz] > 0).to(torch.int32))
            self._dead_row_mask = live == 0
            self._dead_row_mask_version = self.val._version
        return self._dead_row_mask

    @property
    def has_dead_rows(self):
        """True when some row is one of dead_rows.  One device->host sync, once per matrix and state of the values (as
        dead_rows); a fact given through with_facts stays as given."""
        if self._dead_rows is None or self._dead_rows_version not in (None, self.val._version):
            self._dead_rows = bool(self.dead_rows.any().item())
            self._dead_rows_version = self.val._version
        return self._dead_rows

    def quantized(self, qc):
        """The adjacency on the unsigned w_qbits grid (SG.py:626), quantised once per graph and constants."""
        key = _adj_quant_key(qc)
        if key not in self._quantized:
            self._quantized[key] = Csr(self.rowptr, self.col, fake_quantize(self.val, 0, qc.w_qbits, qc.a_s, qc.a_z),
                                       self.n_cols, self._plan).with_facts(flat=self._flat, flat_quant=self._flat_quant)
        return self._quantized[key]

    @property
    def nnz(self):
        return self._nnz

    @property
    def plan(self):
        if self._plan is None:
            self._plan = Plan(self.rowptr)
        return self._plan

    @property
    def gat_plan(self):
        """The schedule for the edge-softmax aggregate: hub rows cut at 256 edges.  Its first stage (the softmax weights,
        csrc/gat_alpha.hip, gat_scan.hip) keeps a row of up to 256 edges in registers -- per row, or per window of stored entries
        on a plan in degree order (the plan's scan_win, built for this cut) -- longer rows go through the plan's tasks.  Measured on
        R-MAT graphs of 2.4 M / 7.5 M / 29 M edges (tools/plan_cut_probe.py): 256 is the best or within 2 % of it for one
        head and for 8, while the plain aggregation prefers 512 / 1024 / 2048 (Plan's default).  The plan also tells the
        library the stored-entry count it sizes the weights with."""
        if getattr(self, "_gat_plan", None) is None:
            self._gat_plan = Plan(self.rowptr, 256, 256)
        return self._gat_plan

    @property
    def wants_plan(self):
        """Building a plan costs one device->host copy and a stream sync; matrices this small finish
        in microseconds on any schedule, so they run without one unless a plan already exists."""
        if self._plan is not None:
            return True
        if self._flat:
            # the entry-split aggregation (sgx_spmm_csr_flat) balances any degree distribution from the entry count alone
            return False
        if self._max_row is not None and self._max_row <= 64 and self.nnz < (1 << 20):
            # known facts (a loader's batch): under 2^20 entries a plan cuts rows over 64 entries and there are none, so
            # it would only reorder short rows -- not worth its read-back, synchronisation and allocations per batch
            return False
        return self.nnz >= 8192

    def with_facts(self, dead_row_mask=None, has_dead_rows=None, max_row=None, flat=None, flat_quant=None):
        """Records what the builder of this matrix already knows, so that nothing is computed or read back for it:
        dead_rows (bool [n_rows]), has_dead_rows, and the longest row (or a bound on it; see wants_plan).
        flat=True: this matrix aggregates by the entry-split form -- ops.spmm takes sgx_spmm_csr_flat for it without
        being asked, and it wants no plan (unless one exists already), whatever its rows are like.
        flat_quant=True: a flat-marked matrix keeps the entry-split route under a quantiser (layer_forward(quant=),
        FPYNQ_GAT with quantisation on); without this fact a flat-marked matrix runs by rows there, as it always did."""
        if flat is not None:
            self._flat = bool(flat)
        if flat_quant is not None:
            self._flat_quant = bool(flat_quant)
        if dead_row_mask is not None:
            self._dead_row_mask, self._dead_row_mask_version = dead_row_mask, None
        if has_dead_rows is not None:
            self._dead_rows, self._dead_rows_version = bool(has_dead_rows), None
        if max_row is not None:
            self._max_row = int(max_row)
        return self

    def to(self, dtype):
        # (the schedule depends on rowptr only: the copy shares this matrix's -- built here if it is wanted and not there
        # yet, so that a copy made per training step does not build one per step)
        if self.val.dtype == dtype:
            return self
        return Csr(self.rowptr, self.col, self.val.to(dtype), self.n_cols,
                   self.plan if self.wants_plan else None).with_facts(max_row=self._max_row, flat=self._flat,
                                                                     flat_quant=self._flat_quant)

    def validate(self):
        check(lib.sgx_csr_validate(_ptr(self.rowptr), _ptr(self.col), self.n_rows, self.n_cols, self.nnz, _stream()),
              "sgx_csr_validate")

    @staticmethod
    def from_dense(dense, dtype=None):
        """Same CSR torch's `_to_sparse_csr()` yields in the molecule notebook (MOL cell 18)."""
        sp = dense.to_sparse_csr()
        val = sp.values() if dtype is None else sp.values().to(dtype)
        return Csr(sp.crow_indices().to(torch.int32).contiguous(), sp.col_indices().to(torch.int32).contiguous(),
                   val.contiguous(), dense.shape[1])

    @staticmethod
    def from_coo(row, col, val, n_rows, n_cols):
        """Edges sorted by row (SG.py ships COO: rowPtr_adj_buffer holds row indices, SG.py:1245)."""
        _dev(row, "row")
        rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=row.device)
        check(lib.sgx_coo_to_csr(_ptr(row.to(torch.int32).contiguous()), row.numel(), n_rows, _ptr(rowptr), _stream()),
              "sgx_coo_to_csr")
        return Csr(rowptr, col.to(torch.int32).contiguous(), val.contiguous(), n_cols)


def csr_from_edge_index(edge_index, n_rows, n_cols=None, values=None, dtype=torch.float16):
    """[2, E] edge list (any order, duplicates add up) -> Csr, without the dense N x N detour of
    `to_dense_adj(...)._to_sparse_csr()` (MOL cell 18): sort by (row, col), merge duplicates,
    row pointer by sgx_coo_to_csr.  Gives the same CSR as the dense route."""
    _dev(edge_index, "edge_index")
    n_cols = n_rows if n_cols is None else n_cols
    key = edge_index[0].to(torch.int64) * n_cols + edge_index[1].to(torch.int64)
    w = torch.ones(key.numel(), dtype=torch.float32, device=key.device) if values is None else values.float()
    ukey, inv = torch.unique(key, return_inverse=True)
    val = torch.zeros(ukey.numel(), dtype=torch.float32, device=key.device).index_add_(0, inv, w)
    row = torch.div(ukey, n_cols, rounding_mode="floor")
    col = ukey - row * n_cols
    keep = val != 0                                     # a dense matrix cannot hold explicit zeros either
    return Csr.from_coo(row[keep].to(torch.int32), col[keep].to(torch.int32), val[keep].to(dtype), n_rows, n_cols)


def _gatherable(H, n_feat=None, nnz=0):
    """The table as the aggregation wants it: rows that start on a dword take 16-byte gathers; a table whose
    rows start on odd halves (47 fp16 columns, unpadded) would be gathered one element per lane, so it is
    copied once into rows of table_pitch() elements -- N x P elements moved against E x P gathered.  A large
    table whose pitch lets rows straddle 128-byte lines (100 halves) is copied too when every row is gathered
    often enough (32 edges per table row) for the 18-25 % the gathers gain to outweigh the copy."""
    n_feat = H.shape[1] if n_feat is None else n_feat
    if not _gatherable_copies(H, n_feat, nnz):
        return H
    padded = torch.empty((H.shape[0], table_pitch(n_feat, H.element_size())), dtype=H.dtype, device=H.device)
    padded[:, :n_feat] = H[:, :n_feat]
    return padded


def _gatherable_copies(H, n_feat, nnz):
    """whether _gatherable copies the table (into fresh rows of table_pitch() elements) instead of passing it on"""
    if (H.stride(0) * H.element_size()) % 4 == 0 and H.data_ptr() % 4 == 0:
        straddles = H.stride(0) != table_pitch(n_feat, H.element_size()) and (H.stride(0) * H.element_size()) % 128 != 0
        return straddles and H.shape[0] * n_feat >= (1 << 22) and nnz >= 32 * H.shape[0]
    return H.shape[0] * n_feat >= (1 << 16)


def spmm(adj, H, relu=False, n_feat=None, out=None, use_plan=True, acc_mode=SGX_ACC_F32, spmm_block=1, schedule=None,
         out_scale=None, requant=None):
    """D = act(A @ H[:, :n_feat]) -- the aggregation stage alone (sgx_spmm_csr).
    schedule="flat", or a matrix that carries the fact (Csr.with_facts(flat=True)): the entry-split form
    (sgx_spmm_csr_flat) -- no plan, no read-back, the grid a function of the entries adj.col holds (a capacity: the
    matrix's own end is read from rowptr on the device), so the call records into a graph and replays.
    out_scale, requant=(scale_fea, internal_bits) (entry-split form only): the quantised layer's store epilogue
    (sgx_spmm_csr_flat_ep) -- float32: D times out_scale, and requantize_ of D, bit for bit; float16 ignores out_scale as
    the row kernels do, and requant raises."""
    if schedule not in (None, "flat"):
        raise ValueError(f"schedule must be None or 'flat', not {schedule!r}")
    flat = schedule == "flat" or adj._flat
    if (out_scale is not None or requant is not None) and not flat:
        raise ValueError("out_scale / requant are the entry-split form's epilogue: pass schedule='flat'")
    if requant is not None and H.dtype != torch.float32:
        raise TypeError("requant works on float32 (SG.py:1545)")
    if flat and acc_mode != SGX_ACC_F32:
        raise ValueError("the entry-split aggregation is SGX_ACC_F32 arithmetic only")
    _dev2d(H, "H")
    n_feat = H.shape[1] if n_feat is None else n_feat
    if acc_mode == SGX_ACC_F32:
        H = _gatherable(H, n_feat, adj.nnz)
    code = dtype_code(H.dtype)
    if adj.val.dtype != H.dtype:
        raise TypeError("adjacency values and H must share one element type (MM.h:129-139)")
    if H.shape[0] < adj.n_cols:
        raise ValueError(f"H has {H.shape[0]} rows, the adjacency refers to {adj.n_cols} columns")
    out = _out(out, adj.n_rows, n_feat, H.dtype, H.device)
    if flat:
        sbytes = lib.sgx_spmm_flat_scratch_bytes(adj.nnz, n_feat)
        scratch = _workspace(H.device, sbytes)
        if out_scale is None and requant is None:
            check(lib.sgx_spmm_csr_flat(code, int(bool(relu)), adj.n_rows, H.shape[0], n_feat, adj.nnz, _ptr(adj.rowptr),
                                        _ptr(adj.col), _ptr(adj.val), _ptr(H), H.stride(0), _ptr(out), out.stride(0), _ptr(scratch),
                                        sbytes, _stream()), "sgx_spmm_csr_flat")
            return out
        scale_fea, internal_bits = (0, 0) if requant is None else (int(requant[0]), int(requant[1]))
        if requant is not None and internal_bits < 1:
            raise ValueError("requant=(scale_fea, internal_bits) needs internal_bits >= 1")
        check(lib.sgx_spmm_csr_flat_ep(code, int(bool(relu)), adj.n_rows, H.shape[0], n_feat, adj.nnz, _ptr(adj.rowptr),
                                       _ptr(adj.col), _ptr(adj.val), _ptr(H), H.stride(0), _ptr(out), out.stride(0), _ptr(scratch),
                                       sbytes, float(out_scale or 0.0), scale_fea, internal_bits, _stream()),
              "sgx_spmm_csr_flat_ep")
        return out
    plan = adj.plan if (use_plan and adj.wants_plan) else None
    sbytes = lib.sgx_spmm_scratch_bytes(plan.handle, n_feat) if plan is not None else 0
    scratch = _workspace(H.device, sbytes) if sbytes else None
    check(lib.sgx_spmm_csr(code, acc_mode, spmm_block, int(bool(relu)), adj.n_rows, H.shape[0], n_feat,
                           _ptr(adj.rowptr), _ptr(adj.col), _ptr(adj.val), _ptr(H), H.stride(0),
                           _ptr(out), out.stride(0), plan.handle if plan is not None else None,
                           _ptr(scratch), sbytes, _stream()), "sgx_spmm_csr")
    return out


def xw_sparse(X, W, out=None, use_plan=True):
    """H = X @ W for a CSR X and a row-major W [M_fea, P] -- the X.W stage alone in gemm_mode 0 (sgx_xw_sparse):
    the weight slice resident in LDS for a large X, gathered through L2 otherwise; same sums either way."""
    _dev2d(W, "W")
    if X.val.dtype != W.dtype:
        raise TypeError("feature values and W must share one element type (MM.h:129-139)")
    if W.shape[0] < X.n_cols:
        raise ValueError(f"W has {W.shape[0]} rows, X refers to {X.n_cols} columns")
    P = W.shape[1]
    W = _gatherable(W, P, X.nnz)
    out = _out(out, X.n_rows, P, W.dtype, W.device)
    plan = X.plan if (use_plan and X.wants_plan) else None
    sbytes = lib.sgx_spmm_scratch_bytes(plan.handle, P) if plan is not None else 0
    scratch = _workspace(W.device, sbytes) if sbytes else None
    check(lib.sgx_xw_sparse(dtype_code(W.dtype), SGX_ACC_F32, 1, X.n_rows, X.n_cols, P, _ptr(X.rowptr), _ptr(X.col),
                            _ptr(X.val), _ptr(W), W.stride(0), _ptr(out), out.stride(0),
                            plan.handle if plan is not None else None, _ptr(scratch), sbytes, _stream()), "sgx_xw_sparse")
    return out


XwSparseForm = collections.namedtuple("XwSparseForm", "lpr n_split full w_vec wgs_per_cu streams")


def xw_sparse_form(X, W, out=None, use_plan=True):
    """Which kernel form xw_sparse(X, W, out) takes (sgx_xw_sparse_form; no launch): None = the gather kernel, otherwise the
    LDS form's arm -- lanes per row, column slices, 16-byte stores, 16-byte fills of W's slice, workgroups per CU, row-tile
    streams of the grid.  The operands are prepared as xw_sparse prepares them, without the copy of W it may make (a copy
    is 16-byte aligned at a pitch of table_pitch() elements, which is all the answer depends on)."""
    _dev2d(W, "W")
    P = W.shape[1]
    if _gatherable_copies(W, P, X.nnz):
        w_ptr, ldw = None, table_pitch(P, W.element_size())
    else:
        w_ptr, ldw = _ptr(W), W.stride(0)
    if out is None:                                         # a fresh [n_rows, P] tensor: aligned, unpadded
        h_ptr, ldh = None, P
    else:
        out = _out(out, X.n_rows, P, W.dtype, W.device)
        h_ptr, ldh = _ptr(out), out.stride(0)
    plan = X.plan if (use_plan and X.wants_plan) else None
    word = lib.sgx_xw_sparse_form(dtype_code(W.dtype), X.n_rows, X.n_cols, P, w_ptr, ldw, h_ptr, ldh,
                                  plan.handle if plan is not None else None)
    if word == 0:
        return None
    return XwSparseForm(word & 0xFF, (word >> 8) & 0xFF, bool(word >> 16 & 1), bool(word >> 17 & 1), (word >> 18) & 3, word >> 20)


def spmm_acc(adj, H, relu=False, acc_in=None, partial_out=False, out=None, use_plan=True):
    """Two-pass aggregation (sgx_spmm_csr_acc): with partial_out the fp32 sums acc_in + A @ H are
    returned; otherwise D = act(acc_in + A @ H) in H's dtype."""
    _dev2d(H, "H")
    n_feat = H.shape[1]
    H = _gatherable(H, n_feat, adj.nnz)
    code = dtype_code(H.dtype)
    if adj.val.dtype != H.dtype:
        raise TypeError("adjacency values and H must share one element type (MM.h:129-139)")
    if H.shape[0] < adj.n_cols:
        raise ValueError(f"H has {H.shape[0]} rows, the adjacency refers to {adj.n_cols} columns")
    if acc_in is not None:
        _dev(acc_in, "acc_in")
        if acc_in.dtype != torch.float32 or acc_in.shape != (adj.n_rows, n_feat):
            raise ValueError("acc_in must be float32 [n_rows, n_feat]")
    acc_out = torch.empty((adj.n_rows, n_feat), dtype=torch.float32, device=H.device) if partial_out else None
    if not partial_out:
        out = _out(out, adj.n_rows, n_feat, H.dtype, H.device)
    plan = adj.plan if (use_plan and adj.wants_plan) else None
    sbytes = lib.sgx_spmm_scratch_bytes(plan.handle, n_feat) if plan is not None else 0
    scratch = _workspace(H.device, sbytes) if sbytes else None
    check(lib.sgx_spmm_csr_acc(code, int(bool(relu)), adj.n_rows, H.shape[0], n_feat, _ptr(adj.rowptr), _ptr(adj.col),
                               _ptr(adj.val), _ptr(H), H.stride(0), None if partial_out else _ptr(out),
                               0 if partial_out else out.stride(0), _ptr(acc_in), _ptr(acc_out), n_feat,
                               plan.handle if plan is not None else None, _ptr(scratch), sbytes, _stream()),
          "sgx_spmm_csr_acc")
    return acc_out if partial_out else out


def table_pitch(width, elem_size):
    """Row pitch (elements) for a table the aggregation gathers from: 16-byte multiples, whole 128-byte lines
    where that costs at most a third more bytes, powers of two below one line (sgx_ldh, csrc/sgx_internal.h)."""
    row = (width * elem_size + 15) // 16 * 16
    if row < 128:
        pitch = 16
        while pitch < row:
            pitch *= 2
    else:
        lines = (row + 127) // 128 * 128
        pitch = lines if 3 * lines <= 4 * row else row
    return pitch // elem_size


def _xw_dense_operands(X, Wt, ldh, out):
    _dev2d(X, "X")
    _dev2d(Wt, "Wt")
    if Wt.dtype != X.dtype or X.shape[1] != Wt.shape[1]:
        raise TypeError(f"X [n, M] and Wt [P, M] must share the element type and M (got {X.dtype} {tuple(X.shape)}, "
                        f"{Wt.dtype} {tuple(Wt.shape)})")
    P = Wt.shape[0]
    if out is not None:
        _out(out, X.shape[0], P, X.dtype, X.device)
        if ldh is not None and ldh != out.stride(0):
            raise ValueError(f"ldh = {ldh} but out has a row stride of {out.stride(0)}")
        return P, out.stride(0)
    return P, (table_pitch(P, X.element_size()) if ldh is None else ldh)


def xw_dense(X, Wt, ldh=None, acc_mode=SGX_ACC_F32, spmm_block=1, relu=False, out=None):
    """H = X @ Wt.T on the matrix cores (sgx_xw_dense).  Wt = weights transposed, [P, M].
    relu: the activation on the stores (sgx_xw_dense_act; the second stage of the aggregate-first order).
    out: a [n, P] view whose row stride is the pitch ldh of H -- ALL ldh elements of each of its rows are written (the
    columns P..ldh-1 with zeros), so the view's rows must own them; the result is `out` itself."""
    P, ldh = _xw_dense_operands(X, Wt, ldh, out)
    M = Wt.shape[1]
    code = dtype_code(X.dtype)
    H = torch.empty((X.shape[0], ldh), dtype=X.dtype, device=X.device) if out is None else out
    if relu:
        if acc_mode != SGX_ACC_F32:
            raise ValueError("the activation rides on the fp32-accumulate kernels only")
        check(lib.sgx_xw_dense_act(code, 1, X.shape[0], M, P, _ptr(X), X.stride(0), _ptr(Wt), Wt.stride(0), _ptr(H), ldh,
                                   _stream()), "sgx_xw_dense_act")
        return H[:, :P]
    check(lib.sgx_xw_dense(code, acc_mode, spmm_block, X.shape[0], M, P, _ptr(X), X.stride(0), _ptr(Wt), Wt.stride(0),
                           _ptr(H), ldh, _stream()), "sgx_xw_dense")
    return H[:, :P]


XW_DENSE_KINDS = ("none", "tile", "stationary", "tile_lds", "wlds", "ref_half")     # SGX_XW_FORM_*
XwDenseForm = collections.namedtuple("XwDenseForm", "kind a b blocks waves vec wgs_per_cu max_trips")


def unpack_xw_dense_form(word, dtype, n_rows):
    """sgx_xw_dense_form's word (include/sgx.h) as an XwDenseForm.  max_trips: the most units of work -- row tiles of one
    column group or block -- one wavefront walks: 1 for the tile kernels, the longest stream's row tiles for the persistent
    grids (tiles of 32 rows in fp16, of 16 in fp32)."""
    if word < 0:
        raise _lib.SgxError(int(word), "sgx_xw_dense_form")
    kind = XW_DENSE_KINDS[word & _lib.SGX_XW_FORM_KIND_MASK]
    a = word >> _lib.SGX_XW_FORM_A_SHIFT & _lib.SGX_XW_FORM_A_MASK
    b = word >> _lib.SGX_XW_FORM_B_SHIFT & _lib.SGX_XW_FORM_B_MASK
    vec = bool(word >> _lib.SGX_XW_FORM_VEC_SHIFT & 1)
    wgs = word >> _lib.SGX_XW_FORM_WGS_SHIFT & _lib.SGX_XW_FORM_WGS_MASK
    blocks = word >> _lib.SGX_XW_FORM_BLOCKS_SHIFT & _lib.SGX_XW_FORM_BLOCKS_MASK
    waves = word >> _lib.SGX_XW_FORM_WAVES_SHIFT
    tiles = -(-n_rows // (32 if dtype == torch.float16 else 16))
    if kind == "stationary":
        trips = -(-tiles // (waves // blocks))
    elif kind == "wlds":
        trips = -(-tiles // waves)
    else:
        trips = 1 if kind in ("tile", "tile_lds") else 0
    return XwDenseForm(kind, a, b, blocks, waves, vec, wgs, trips)


def xw_dense_form(X, Wt, ldh=None, acc_mode=SGX_ACC_F32, out=None):
    """Which kernel arm xw_dense(X, Wt, ldh, acc_mode, out=out) takes (sgx_xw_dense_form; no launch): the kind, its template
    arguments a, b, the column blocks or groups, the wavefronts of the grid, whether H leaves in vector stores, the
    workgroups per CU and max_trips.  Without `out` the result is a fresh allocation: aligned at any pitch."""
    P, ldh = _xw_dense_operands(X, Wt, ldh, out)
    h_ptr = ctypes.c_void_p(256) if out is None else _ptr(out)
    n = X.shape[0]
    word = lib.sgx_xw_dense_form(dtype_code(X.dtype), acc_mode, n, Wt.shape[1], P, _ptr(X) if n else None, X.stride(0), _ptr(Wt),
                                 Wt.stride(0), h_ptr if n else None, ldh)
    return unpack_xw_dense_form(word, X.dtype, n)


def transpose(x, ldo=None):
    _dev(x, "x")
    rows, cols = x.shape
    ldo = rows if ldo is None else ldo
    out = torch.empty((cols, ldo), dtype=x.dtype, device=x.device)
    check(lib.sgx_transpose(dtype_code(x.dtype), rows, cols, _ptr(x), x.stride(0), _ptr(out), ldo, _stream()),
          "sgx_transpose")
    return out


def layer_forward(adj, fea, Wt, relu=False, gat_attention=None, alpha=0.2, want_edge_outputs=False, quant_int8=False,
                  acc_mode=SGX_ACC_F32, spmm_block=1, bias_count=0, out=None, use_plan=True, agg_events=None,
                  quant=None, adj_quantized=False, cache_quantized_adj=True, fea_threads=1, adj_threads=1,
                  gat_heads=1, order="reference", want_row_stats=False, schedule=None, fill_dead_rows=None,
                  quant_flat=False, _schedule_query=False):
    """One fused layer  D = act(A . (X . W))  through sgx_layer_forward.

    adj : Csr [N, M_adj];  fea : Csr [M_adj, M_fea] (gemm_mode 0) or dense tensor (gemm_mode 1);
    Wt  : [P, M_fea] -- the weights TRANSPOSED, what the reference writes into B_buffer.
    Returns D [N, P] (and (E, S) per-edge tensors when want_edge_outputs with GAT).
    want_row_stats (GAT, instead of want_edge_outputs): returns (D, GatStats) through sgx_layer_forward_stats -- the row
    softmax statistics that stand for E and S; D is the layer's D without side outputs, bit for bit.
    quant: a quant.QuantConstants -- run the layer with the quantised arithmetic of the SGRACE
    bitstream (fp32 tensors only); quant_int8: with dense features, X and W go to the int8 matrix cores as the integer
    codes of their grids (SGX_QUANT_INT8: exact int32 sums, X read as bytes), "auto" = where that is the faster form
    (SGX_QUANT_INT8_AUTO: M_fea > 128); adj_quantized: adj.val already went through the quantiser;
    cache_quantized_adj: quantise the adjacency once per graph on the host side instead of inside
    every call (always done for GAT, whose mask decides how rows without a live edge are treated).
    order: "reference" -- X.W first, as the reference's dataflow; "aggregate_first" -- D = act((A.X).W), which
    gathers M_fea instead of P columns per edge (dense X, GCN aggregate, default arithmetic only); "auto" --
    aggregate first where that is allowed and M_fea < P.
    A square dense fp16 layer (M_fea = P = 64, GCN aggregate, default arithmetic) runs as ONE launch under every order:
    the aggregation of X with W applied in its epilogue, D = act(f16(A.X).W), bit-equal to "aggregate_first" run as two
    launches.  "reference" may apply W after the aggregation for that shape -- both associations gather 64 columns per
    edge and the default arithmetic follows the reference within a tolerance, not bit for bit (SGX_ACC_REF_HALF does and
    keeps X.W first).  Plans that cut rows or reorder them, tables of 4 GiB and more and SGX_LAYER_NO_FUSED_DENSE in the
    environment keep the staged launches (include/sgx.h, sgx_layer_desc.order).
    schedule="flat", or an adjacency that carries the fact (Csr.with_facts(flat=True)): the aggregate stage on the
    entry-split schedule (SGX_SCHEDULE_FLAT, nnz_adj = adj.nnz, the entries adj.col holds: a capacity) -- no plan is looked
    up, nothing is read back, so the layer records into a graph and replays on another adjacency of the same capacity; D is
    bit-equal to the X.W stage call followed by spmm / gat_aggregate(schedule="flat").  The keyword together with quant,
    gat_heads > 1, SGX_ACC_REF_HALF, want_edge_outputs or order="aggregate_first" raises; a flat-marked adjacency with one of
    them runs as without the fact.  A flat-marked feature CSR on that route has its X.W stage run as spmm(fea, W,
    schedule="flat") -- a CSR X.W is an aggregation over W -- and the layer is then the two stage calls, composed here.
    quant_flat=True: the quantised layer's own opt-in to that schedule (SGX_QUANT_FLAT): schedule="flat" with quant= is then
    taken instead of refused -- stage 1 as under the default schedule, stage 2 the entry-split aggregate with deq_o on its
    stores; D equals the stage calls composed (include/sgx.h).  An adjacency marked with_facts(flat=True, flat_quant=True)
    opts in by itself; one marked flat alone still runs a quantised layer by rows.  The other refusals stay.
    fill_dead_rows (GAT): None = decide from the adjacency (adj.has_dead_rows: a read-back unless the fact is known), or the
    rule itself, as gat_aggregate takes it.
    """
    if schedule not in (None, "flat"):
        raise ValueError(f"schedule must be None or 'flat', not {schedule!r}")
    quant_ok = bool(quant_flat) or (schedule is None and adj._flat and adj._flat_quant)
    refused = [name for name, hit in (("quant", quant is not None and not quant_ok), ("gat_heads > 1", int(gat_heads) > 1),
                                      ("SGX_ACC_REF_HALF", acc_mode != SGX_ACC_F32), ("want_edge_outputs", want_edge_outputs),
                                      ("order='aggregate_first'", order == "aggregate_first")) if hit]
    if schedule == "flat" and refused:
        raise ValueError(f"the entry-split schedule does not go with {', '.join(refused)} (sgx_layer_desc.schedule_adj)")
    flat = schedule == "flat" or (adj._flat and not refused)
    if flat and isinstance(fea, Csr) and fea._flat:
        if _schedule_query:
            return 2
        return _layer_forward_flat_stages(adj, fea, Wt, relu, gat_attention, alpha, bias_count, out, agg_events, want_row_stats,
                                          fill_dead_rows, quant, adj_quantized)
    _dev(Wt, "Wt")
    code = dtype_code(Wt.dtype)
    P, M_fea = Wt.shape
    d = LayerDesc()
    gemm_mode = 0 if isinstance(fea, Csr) else 1
    if order not in ("reference", "aggregate_first", "auto"):
        raise ValueError(f"order must be 'reference', 'aggregate_first' or 'auto', not {order!r}")
    can_swap = gemm_mode == 1 and gat_attention is None and quant is None and acc_mode == SGX_ACC_F32
    if order == "aggregate_first" and not can_swap:
        raise ValueError("aggregate_first needs dense features, the GCN aggregate and the default arithmetic "
                         "(no GAT, no quantised layer, no SGX_ACC_REF_HALF)")
    swap = order == "aggregate_first" or (order == "auto" and can_swap and M_fea < P and not flat)
    d.order = SGX_ORDER_AGGREGATE_FIRST if swap else SGX_ORDER_REFERENCE
    d.gemm_mode, d.relu, d.gat_mode = gemm_mode, int(bool(relu)), int(gat_attention is not None)
    d.N_adj, d.M_adj, d.M_fea, d.P_w = adj.n_rows, adj.n_cols, M_fea, P
    d.bias_count, d.dtype, d.acc_mode, d.spmm_block = bias_count, code, acc_mode, spmm_block
    d.fea_threads, d.adj_threads = int(fea_threads), int(adj_threads)      # observable in SGX_ACC_REF_HALF only
    if adj.val.dtype != Wt.dtype:
        raise TypeError("adjacency, features and weights must share one element type (MM.h:129-139)")
    if quant is not None and Wt.dtype != torch.float32:
        raise TypeError("the quantised layer works on float32 buffers (SG.py:1545)")
    if gemm_mode == 0:
        if fea.val.dtype != Wt.dtype or fea.n_rows != adj.n_cols or fea.n_cols != M_fea:
            raise ValueError("feature CSR does not match adjacency / weights")
        d.rowPtr_fea, d.columnIndex_fea, d.values_fea = (fea.rowptr.data_ptr(), fea.col.data_ptr(),
                                                         fea.val.data_ptr())
        if use_plan and fea.wants_plan:
            d.plan_fea = fea.plan.handle
    else:
        _dev(fea, "fea")
        if fea.dtype != Wt.dtype or fea.shape != (adj.n_cols, M_fea):
            raise ValueError(f"dense features must be [{adj.n_cols}, {M_fea}] {Wt.dtype}")
        d.values_fea = fea.data_ptr()
    if quant is not None and not adj_quantized and (cache_quantized_adj or gat_attention is not None):
        adj, adj_quantized = adj.quantized(quant), True
    if gat_attention is not None:
        d.gat_fill_dead_rows = int(adj.has_dead_rows if fill_dead_rows is None else bool(fill_dead_rows))
    d.rowPtr_adj, d.columnIndex_adj, d.values_adj = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.val.data_ptr()
    if flat:
        d.schedule_adj, d.nnz_adj = _lib.SGX_SCHEDULE_FLAT, adj.nnz
    elif use_plan and adj.wants_plan:
        d.plan_adj = (adj.gat_plan if gat_attention is not None else adj.plan).handle
    d.B = Wt.data_ptr()
    out = _out(out, adj.n_rows, P, Wt.dtype, Wt.device)
    if out.stride(0) != P:
        raise ValueError("the layer writes D densely ([N_adj][P_w], K.cpp:802): `out` must not have padded rows")
    d.D = out.data_ptr()
    E = S = None
    if want_row_stats and (want_edge_outputs or gat_attention is None):
        raise ValueError("want_row_stats needs the GAT aggregate and excludes want_edge_outputs")
    if gat_attention is not None:
        att = _dev(gat_attention, "attention").reshape(-1)
        if att.numel() != 2 * P or att.dtype != Wt.dtype:
            raise ValueError("attention must hold 2*P_w elements of the layer dtype")
        d.attention, d.alpha = att.data_ptr(), float(alpha)
        if P % int(gat_heads):
            raise ValueError("P_w must be a multiple of gat_heads")
        d.gat_heads = int(gat_heads)
        if want_edge_outputs:
            es_shape = (adj.nnz,) if gat_heads == 1 else (adj.nnz, int(gat_heads))
            E = torch.empty(es_shape, dtype=torch.float32, device=Wt.device)
            S = torch.empty(es_shape, dtype=torch.float32, device=Wt.device)
            d.E, d.S = E.data_ptr(), S.data_ptr()
    if agg_events is not None:          # (begin, end) hipEvent_t handles, see hipevents.py
        d.ev_agg_begin, d.ev_agg_end = agg_events
    if quant is not None:
        qs = quant.as_struct(nnz_adj=adj.nnz, nnz_fea=fea.nnz if gemm_mode == 0 else 0, adj_done=adj_quantized)
        if quant_int8 == "auto":
            qs.flags |= _lib.SGX_QUANT_INT8_AUTO
        elif quant_int8:
            qs.flags |= _lib.SGX_QUANT_INT8
        if flat:
            qs.flags |= _lib.SGX_QUANT_FLAT
        d.quant = ctypes.pointer(qs)
    if _schedule_query:
        route = lib.sgx_layer_schedule(ctypes.byref(d))
        if route < 0:
            check(int(route), "sgx_layer_schedule")
        return int(route)
    nbytes = lib.sgx_layer_workspace_bytes(ctypes.byref(d))
    ws = _workspace(Wt.device, nbytes)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if want_row_stats:
        stats = GatStats(adj.n_rows, adj.n_cols, gat_heads, Wt.device)
        st = stats.struct()
        check(lib.sgx_layer_forward_stats(ctypes.byref(d), ctypes.byref(st), _stream()), "sgx_layer_forward_stats")
        return out, stats
    check(lib.sgx_layer_forward(ctypes.byref(d), _stream()), "sgx_layer_forward")
    return (out, E, S) if want_edge_outputs else out


def layer_schedule(adj, fea, Wt, **kwargs):
    """Which schedule the aggregate stage of layer_forward(adj, fea, Wt, **kwargs) takes (sgx_layer_schedule; no launch):
    0 = by rows without a plan, 1 = by rows with the adjacency's plan, 2 = entry-split.  The operands are prepared as
    layer_forward prepares them (a plan the call would build is built)."""
    return layer_forward(adj, fea, Wt, _schedule_query=True, **kwargs)


def _layer_forward_flat_stages(adj, fea, Wt, relu, gat_attention, alpha, bias_count, out, agg_events, want_row_stats,
                               fill_dead_rows, quant=None, adj_quantized=False):
    """layer_forward on the entry-split schedule for a flat-marked feature CSR: sgx_layer_forward has one X.W stage for a
    CSR X (sgx_xw_sparse) and no way to take an H formed elsewhere, so the layer is its two stage calls -- H = spmm(fea,
    W, schedule="flat") into rows of table_pitch() elements, then the entry-split aggregate of H -- and D is theirs bit for
    bit.  quant: the same composition on the quantised operands -- W and the attention vector on the
    signed grid, the stored values of X and A on the unsigned one (A once per matrix, Csr.quantized), the requantisation on
    the stores of the X.W stage and deq_o on the aggregate's."""
    _dev(Wt, "Wt")
    P, M_fea = Wt.shape
    if quant is not None and Wt.dtype != torch.float32:
        raise TypeError("the quantised layer works on float32 buffers (SG.py:1545)")
    if adj.val.dtype != Wt.dtype:
        raise TypeError("adjacency, features and weights must share one element type (MM.h:129-139)")
    if fea.val.dtype != Wt.dtype or fea.n_rows != adj.n_cols or fea.n_cols != M_fea:
        raise ValueError("feature CSR does not match adjacency / weights")
    if want_row_stats and gat_attention is None:
        raise ValueError("want_row_stats needs the GAT aggregate and excludes want_edge_outputs")
    out = _out(out, adj.n_rows, P, Wt.dtype, Wt.device)
    if out.stride(0) != P:
        raise ValueError("the layer writes D densely ([N_adj][P_w], K.cpp:802): `out` must not have padded rows")
    if bias_count > 0:                      # K.cpp:3876-3889: the reference preloads and returns without computing
        return (out, GatStats(adj.n_rows, adj.n_cols, 1, Wt.device)) if want_row_stats else out
    ldh = table_pitch(P, Wt.element_size())
    requant = deq_o = None
    if quant is not None:
        if quant.a_z != 0 or quant.f_z != 0:       # (sgx_layer_forward's rule: entries that are not stored must stay zero)
            raise ValueError("the quantised layer needs zero points a_z = f_z = 0 for its CSR operands")
        Wt = fake_quantize(Wt.contiguous(), 1, quant.w_qbits, quant.w_s, quant.w_z)
        fea = Csr(fea.rowptr, fea.col, fake_quantize(fea.val, 0, quant.w_qbits, quant.f_s, quant.f_z), fea.n_cols)
        if not adj_quantized:
            adj = adj.quantized(quant)
        if gat_attention is not None:
            gat_attention = fake_quantize(_dev(gat_attention, "attention").reshape(-1).contiguous(), 1, quant.w_qbits, quant.w_s,
                                          quant.w_z)
        requant, deq_o = (quant.scale_fea, quant.internal_quantization), quant.deq_o
    W = transpose(Wt, ldo=ldh)                                              # B [P][M] -> W [M][ldh]
    H = torch.zeros((adj.n_cols, ldh), dtype=Wt.dtype, device=Wt.device)
    spmm(fea, W, n_feat=P, out=H[:, :P], schedule="flat", requant=requant)
    if agg_events is not None:
        check(lib.sgx_event_record(agg_events[0], _stream()), "sgx_event_record")
    if gat_attention is None:
        res = spmm(adj, H, relu=relu, n_feat=P, out=out, schedule="flat", out_scale=deq_o)
    else:
        res = gat_aggregate(adj, H[:, :P], gat_attention, alpha=alpha, relu=relu, fill_dead_rows=fill_dead_rows, out=out,
                            want_row_stats=want_row_stats, schedule="flat", out_scale=deq_o)
    if agg_events is not None:
        check(lib.sgx_event_record(agg_events[1], _stream()), "sgx_event_record")
    return res


def fake_quantize(x, signed, qbits, scale, zero, out=None):
    """quantization_fbits (signed) / quantization_ufbits (SG.py:238-265) of an fp32 tensor on the device."""
    _dev(x, "x")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("fake_quantize works on contiguous float32 tensors (SG.py:1545)")
    if out is None:
        out = torch.empty_like(x)
    check(lib.sgx_fake_quantize(int(bool(signed)), int(qbits), float(1 / scale), float(zero), x.numel(), _ptr(x), _ptr(out),
                                _stream()), "sgx_fake_quantize")
    return out


def quantize_codes_i8(x, signed, qbits, scale, zero):
    """The integer codes of an fp32 matrix on its w_qbits grid as int8 [rows, pitch] (pitch = columns rounded up to
    16, pad codes 0); unsigned 8-bit codes are stored minus 128 (sgx_quantize_codes_i8).  Returns (codes, bias)."""
    _dev2d(x, "x")
    if x.dtype != torch.float32:
        raise TypeError("codes are taken from float32 values (SG.py:1545)")
    n, m = x.shape
    ldc = (m + 15) // 16 * 16
    codes = torch.empty((n, ldc), dtype=torch.int8, device=x.device)
    check(lib.sgx_quantize_codes_i8(int(bool(signed)), int(qbits), float(1 / scale), float(zero), n, m, _ptr(x), x.stride(0),
                                    _ptr(codes), ldc, _stream()), "sgx_quantize_codes_i8")
    return codes, lib.sgx_code_bias(int(bool(signed)), int(qbits))


def xw_dense_i8(Xc, Wc, M_fea, qbits, scale_fea=0, internal_bits=0):
    """H = requant((Xc . Wc^T + bias terms) / 2^(2(qbits-1))) on the int8 matrix cores (sgx_xw_dense_i8): Xc unsigned
    feature codes [n, pitch], Wc signed weight codes [P, pitch] as quantize_codes_i8 returns them."""
    n, P = Xc.shape[0], Wc.shape[0]
    H = torch.empty((n, P), dtype=torch.float32, device=Xc.device)
    ws = torch.empty(max(1, lib.sgx_xw_dense_i8_workspace_bytes(P)), dtype=torch.uint8, device=Xc.device)
    check(lib.sgx_xw_dense_i8(int(qbits), n, int(M_fea), P, _ptr(Xc), Xc.stride(0), _ptr(Wc), Wc.stride(0), int(scale_fea),
                              int(internal_bits), _ptr(H), H.stride(0), _ptr(ws), _stream()), "sgx_xw_dense_i8")
    return H


def requantize_(H, scale_fea, internal_bits):
    """H <- round_decimals(clip(H / 2^scale_fea), internal_bits - 1) in place (SG.py:607-616)."""
    _dev2d(H, "H")
    if H.dtype != torch.float32:
        raise TypeError("requantize_ works on float32")
    check(lib.sgx_requantize(H.shape[0], H.shape[1], H.stride(0), _ptr(H), int(scale_fea), int(internal_bits), _stream()),
          "sgx_requantize")
    return H


def _check_fill_row(fill_row, F, n_nodes):
    _dev(fill_row, "fill_row")
    if fill_row.dtype != torch.float32 or fill_row.numel() != F or not n_nodes:
        raise ValueError("fill_row must be float32 [F] and come with n_nodes")


def gat_aggregate(adj, Wh, attention, alpha=0.2, relu=False, want_edge_outputs=False, fill_dead_rows=None, out=None,
                  heads=1, use_plan=True, fill_row=None, n_nodes=None, want_row_stats=False, schedule=None, out_scale=None):
    """Edge-softmax aggregate over an already computed Wh [adj.n_cols, F]; row r of adj is node r of Wh.
    heads > 1: F/heads columns per head, attention = heads vectors of 2*F/heads (E, S become [nnz, heads]).
    fill_dead_rows: None = decide from the adjacency (rows without a positive entry get the mean of
    all rows of Wh, as in the reference's dense emulation), False = such rows give 0.
    fill_row (fp32 [F]) with n_nodes: one rank of a partitioned graph -- dead rows receive this row (the mean over
    ALL nodes, reduced across ranks by the caller) and S = 1/n_nodes (sgx_gat_aggregate_fill).
    want_row_stats (instead of want_edge_outputs): returns (out, GatStats) through sgx_gat_aggregate_stats; `out` is what
    the call without side outputs gives on the same arguments, bit for bit.
    schedule="flat", or a matrix that carries the fact (Csr.with_facts(flat=True)): the entry-split form
    (sgx_gat_aggregate_flat) -- one head, no edge outputs, no plan, no read-back, the grid a function of the entries
    adj.col holds (a capacity), so the call records into a graph and replays; a caller that replays passes fill_dead_rows
    itself.  The keyword with heads > 1 or want_edge_outputs raises; a flat-marked matrix with them runs as without the fact.
    out_scale (entry-split form only): the quantised layer's deq_o on the stores (sgx_gat_aggregate_flat_ep) -- float32: D
    times out_scale bit for bit, the statistics unchanged; float16 ignores it as the row kernels do."""
    if schedule not in (None, "flat"):
        raise ValueError(f"schedule must be None or 'flat', not {schedule!r}")
    heads = int(heads)
    if schedule == "flat" and (heads != 1 or want_edge_outputs):
        raise ValueError("the entry-split GAT aggregate has one head and no edge outputs (want_row_stats gives the statistics)")
    flat = schedule == "flat" or (adj._flat and heads == 1 and not want_edge_outputs)
    if out_scale is not None and not flat:
        raise ValueError("out_scale is the entry-split form's epilogue: pass schedule='flat'")
    _dev2d(Wh, "Wh")
    code = dtype_code(Wh.dtype)
    N, F = Wh.shape
    if N != adj.n_cols or adj.n_rows > N:
        raise ValueError(f"Wh must have adj.n_cols = {adj.n_cols} rows (got {N}) and adj.n_rows <= adj.n_cols")
    att = _dev(attention, "attention").reshape(-1)
    if adj.val.dtype != Wh.dtype or att.dtype != Wh.dtype:
        raise TypeError("adjacency values, Wh and the attention vector must share one element type (MM.h:129-139)")
    out = _out(out, adj.n_rows, F, Wh.dtype, Wh.device)
    E = S = None
    if F % heads or att.numel() != 2 * F:
        raise ValueError("F must be a multiple of heads and attention must hold 2*F elements")
    if want_edge_outputs:
        es_shape = (adj.nnz,) if heads == 1 else (adj.nnz, heads)
        E = torch.empty(es_shape, dtype=torch.float32, device=Wh.device)
        S = torch.empty(es_shape, dtype=torch.float32, device=Wh.device)
    if flat:
        return _gat_aggregate_flat(adj, Wh, att, alpha, relu, fill_dead_rows, out, fill_row, n_nodes, want_row_stats, out_scale)
    plan = adj.gat_plan.handle if (use_plan and adj.wants_plan) else None
    if want_row_stats:
        return _gat_aggregate_stats(adj, Wh, att, alpha, relu, want_edge_outputs, fill_dead_rows, out, heads, plan, fill_row,
                                    n_nodes)
    if fill_row is not None:
        _check_fill_row(fill_row, F, n_nodes)
        s = torch.empty(lib.sgx_gat_scratch_bytes(N, F, heads, 0, plan) // 4, dtype=torch.float32, device=Wh.device)
        check(lib.sgx_gat_aggregate_fill(code, int(bool(relu)), adj.n_rows, N, F, heads, float(alpha), _ptr(adj.rowptr),
                                         _ptr(adj.col), _ptr(adj.val), _ptr(Wh), Wh.stride(0), _ptr(att), _ptr(out),
                                         out.stride(0), _ptr(E), _ptr(S), _ptr(fill_row.contiguous()), int(n_nodes), plan,
                                         _ptr(s), _stream()), "sgx_gat_aggregate_fill")
        return (out, E, S) if want_edge_outputs else out
    fill = int(adj.has_dead_rows if fill_dead_rows is None else bool(fill_dead_rows))
    s = torch.empty(lib.sgx_gat_scratch_bytes(N, F, heads, fill, plan) // 4, dtype=torch.float32, device=Wh.device)
    check(lib.sgx_gat_aggregate(code, int(bool(relu)), fill, adj.n_rows, N, F, heads, float(alpha), _ptr(adj.rowptr), _ptr(adj.col),
                                _ptr(adj.val), _ptr(Wh), Wh.stride(0), _ptr(att), _ptr(out), out.stride(0),
                                _ptr(E), _ptr(S), plan, _ptr(s), _stream()), "sgx_gat_aggregate")
    return (out, E, S) if want_edge_outputs else out


def _gat_aggregate_stats(adj, Wh, att, alpha, relu, want_edge_outputs, fill_dead_rows, out, heads, plan, fill_row, n_nodes):
    """gat_aggregate(..., want_row_stats=True) on its checked arguments: sgx_gat_aggregate_stats, whose fill / n_nodes pair
    selects the dead-row rule (a fill row; n_nodes = 0: zero; n_nodes = n_cols: the mean of Wh's rows)."""
    if want_edge_outputs:
        raise ValueError("want_row_stats and want_edge_outputs exclude each other")
    N, F = Wh.shape
    if fill_row is not None:
        _check_fill_row(fill_row, F, n_nodes)
        fill, nn = 0, int(n_nodes)
    else:
        fill = int(adj.has_dead_rows if fill_dead_rows is None else bool(fill_dead_rows))
        nn = N if fill else 0
    s = torch.empty(lib.sgx_gat_scratch_bytes(N, F, heads, fill, plan) // 4, dtype=torch.float32, device=Wh.device)
    stats = GatStats(adj.n_rows, N, heads, Wh.device)
    st = stats.struct()
    check(lib.sgx_gat_aggregate_stats(dtype_code(Wh.dtype), int(bool(relu)), adj.n_rows, N, F, heads, float(alpha),
                                      _ptr(adj.rowptr), _ptr(adj.col), _ptr(adj.val), _ptr(Wh), Wh.stride(0), _ptr(att),
                                      _ptr(out), out.stride(0), _ptr(fill_row), nn, plan, _ptr(s), ctypes.byref(st), _stream()),
          "sgx_gat_aggregate_stats")
    return out, stats


def _gat_aggregate_flat(adj, Wh, att, alpha, relu, fill_dead_rows, out, fill_row, n_nodes, want_row_stats, out_scale=None):
    """gat_aggregate on its checked arguments through sgx_gat_aggregate_flat: the dead-row rule as _gat_aggregate_stats maps
    it, the scratch from the grow-only workspace, nnz = the entries adj.col holds."""
    N, F = Wh.shape
    if fill_row is not None:
        _check_fill_row(fill_row, F, n_nodes)
        fill_row = fill_row.contiguous()
        mean_rule, nn = 0, int(n_nodes)
    else:
        mean_rule = int(adj.has_dead_rows if fill_dead_rows is None else bool(fill_dead_rows))
        nn = N if mean_rule else 0
    sbytes = lib.sgx_gat_flat_scratch_bytes(adj.nnz, adj.n_rows, N, F, mean_rule)
    scratch = _workspace(Wh.device, sbytes)
    stats = GatStats(adj.n_rows, N, 1, Wh.device) if want_row_stats else None
    st = stats.struct() if stats is not None else None
    args = (dtype_code(Wh.dtype), int(bool(relu)), adj.n_rows, N, F, 1, float(alpha), adj.nnz, _ptr(adj.rowptr), _ptr(adj.col),
            _ptr(adj.val), _ptr(Wh), Wh.stride(0), _ptr(att), _ptr(out), out.stride(0), _ptr(fill_row), nn, _ptr(scratch), sbytes,
            ctypes.byref(st) if st is not None else None)
    if out_scale is None:
        check(lib.sgx_gat_aggregate_flat(*args, _stream()), "sgx_gat_aggregate_flat")
    else:
        check(lib.sgx_gat_aggregate_flat_ep(*args, float(out_scale), _stream()), "sgx_gat_aggregate_flat_ep")
    return (out, stats) if want_row_stats else out


def col_sums(X, n_feat=None):
    """fp32 column sums of the rows of X [n, F] in a fixed order (sgx_col_sums): a rank's share of the mean row the
    partitioned GAT layer gives rows without a live edge."""
    _dev2d(X, "X")
    F = X.shape[1] if n_feat is None else n_feat
    out = torch.empty(F, dtype=torch.float32, device=X.device)
    scratch = torch.empty(lib.sgx_col_sums_scratch_bytes(F) // 4, dtype=torch.float32, device=X.device)
    check(lib.sgx_col_sums(dtype_code(X.dtype), X.shape[0], F, _ptr(X), X.stride(0), _ptr(out), _ptr(scratch), _stream()),
          "sgx_col_sums")
    return out


def pack_rows(src, row_index, out=None, stream=None):
    """out[i] = src[row_index[i]] (sgx_pack_rows): the rows of H a peer asked for, gathered into the send buffer of
    the halo exchange.  row_index int32 on the device; stream: a torch stream other than the current one to launch on."""
    _dev2d(src, "src")
    _dev(row_index, "row_index")
    if row_index.dtype != torch.int32:
        raise TypeError("row_index must be int32")
    n, F = row_index.numel(), src.shape[1]
    out = _out(out, n, F, src.dtype, src.device)
    st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    check(lib.sgx_pack_rows(dtype_code(src.dtype), n, F, _ptr(src), src.stride(0), _ptr(row_index), _ptr(out), out.stride(0), st),
          "sgx_pack_rows")
    return out


def xt_g(X, G):
    """grad_W = X^T @ G (sgx_xt_g): X [n, M] fp16|fp32 dense, G [n, P] fp32 -> [M, P] fp32."""
    _dev2d(X, "X")
    _dev2d(G, "G")
    if G.dtype != torch.float32:
        raise TypeError("G must be float32 (the backward pass runs in fp32, MOL cell 16)")
    n, M = X.shape
    P = G.shape[1]
    out = torch.empty((M, P), dtype=torch.float32, device=X.device)
    nbytes = lib.sgx_xt_g_workspace_bytes(n, M, P)
    ws = _workspace(X.device, nbytes)
    check(lib.sgx_xt_g(dtype_code(X.dtype), n, M, P, _ptr(X), X.stride(0), _ptr(G), G.stride(0), _ptr(out), P,
                       _ptr(ws), ws.numel(), _stream()), "sgx_xt_g")
    return out


# the form csr_transpose(method=None) takes: "device" (sgx_csr_transpose) or "torch" (sort plumbing); DESIGN 4.13 holds the
# measurement that chose it
CSR_TRANSPOSE_DEFAULT = "device"


def _transposed(T, return_order, order, flat=False, flat_quant=False):
    if flat_quant:
        T.with_facts(flat_quant=True)
    if flat:
        # the transpose of an entry-split matrix is one: no plan for it, whatever its rows (a hub column's) are like
        T.with_facts(flat=True)
    elif T.n_rows > 0 and T.nnz >= 64 * T.n_rows:
        # a feature matrix transposed: a handful of rows, each as long as the graph is wide (MUTAG: 7 rows of ~500 entries) --
        # below the size at which a plan is built by itself, and exactly the shape that needs one: without it 7 lane groups
        # walk 60 dependent steps each (58 us for a 3.4 K-entry matrix) where the plan's 64-edge tasks take a few
        T.plan
    return (T, order) if return_order else T


def csr_transpose(A, return_order=False, method=None):
    """CSR of A^T (values kept, same dtype); features are fixed across epochs, so callers cache it.
    return_order: also the edge permutation (edge k of A^T is edge order[k] of A), int64.
    method: "device" -- sgx_csr_transpose, the stable transpose of include/sgx.h in four launches per sort pass and no
    synchronisation; "torch" -- the int64 key, argsort and gathers this function was before; None -- CSR_TRANSPOSE_DEFAULT.
    On a matrix that stores every (row, col) pair once both give the same arrays; copies of a pair keep their source order
    on the device and stand in no defined order under "torch".
    The transpose of a flat-marked matrix (Csr.with_facts(flat=True)) is flat-marked and no plan is built for it."""
    method = CSR_TRANSPOSE_DEFAULT if method is None else method
    if method == "device":
        nnz, dev = A.nnz, A.rowptr.device
        rowptr_t = torch.empty(A.n_cols + 1, dtype=torch.int32, device=dev)
        col_t = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        val_t = torch.empty(max(nnz, 1), dtype=A.val.dtype, device=dev)
        order = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev) if return_order else None
        ws = _workspace(dev, lib.sgx_csr_transpose_workspace_bytes(A.n_rows, A.n_cols, nnz))
        check(lib.sgx_csr_transpose(dtype_code(A.val.dtype), A.n_rows, A.n_cols, nnz, _ptr(A.rowptr), _ptr(A.col), _ptr(A.val),
                                    _ptr(rowptr_t), _ptr(col_t), _ptr(val_t), _ptr(order), _ptr(ws), ws.numel(), _stream()),
              "sgx_csr_transpose")
        T = Csr(rowptr_t, col_t[:nnz], val_t[:nnz], A.n_rows)
        return _transposed(T, return_order, order[:nnz].long() if return_order else None, A._flat, A._flat_quant)
    if method != "torch":
        raise ValueError(f"csr_transpose: method must be None, 'device' or 'torch', not {method!r}")
    row = torch.repeat_interleave(torch.arange(A.n_rows, device=A.col.device, dtype=torch.int64),
                                  (A.rowptr[1:] - A.rowptr[:-1]).long(), output_size=A.nnz)
    col, val = A.col[:A.nnz], A.val[:A.nnz]
    key = col.to(torch.int64) * A.n_rows + row
    order = torch.argsort(key)
    T = Csr.from_coo(col[order].contiguous(), row[order].to(torch.int32).contiguous(), val[order].contiguous(),
                     A.n_cols, A.n_rows)
    return _transposed(T, return_order, order, A._flat, A._flat_quant)


def _backward_edge_operands(adj, G, Wh, dead):
    """What both backward edge passes hand the kernel beside G: (dead_rs, Wh) -- the dead rows' softmax row sum
    G[r] . mean(Wh) (None without `dead`), and Wh with rows the kernel can gather 16 bytes at a time."""
    dead_rs = None
    if dead is not None:
        _dev(dead, "dead")
        if dead.dtype != torch.bool or dead.shape != (adj.n_rows,):
            raise ValueError("dead must be a bool [adj.n_rows] tensor")
        wh_mean = (col_sums(Wh) / adj.n_cols).unsqueeze(0)                   # [1, F]
        dead_rs = xw_dense(G if G.stride(0) == G.shape[1] else G.contiguous(), wh_mean)[:, 0].contiguous()
    if Wh.stride(0) % 4 or Wh.data_ptr() % 16:           # rows are gathered 16 bytes at a time: pad them
        padded = torch.zeros((Wh.shape[0], (Wh.shape[1] + 3) // 4 * 4), dtype=torch.float32, device=Wh.device)
        padded[:, :Wh.shape[1]] = Wh
        Wh = padded[:, :Wh.shape[1]]
    return dead_rs, Wh


def gat_backward_edges(adj, E, S, G, Wh, alpha=0.2, dead=None):
    """Edge pass of FPYNQ_GAT.backward (sgx_gat_backward_edges): returns (sg [nnz], g1 [n_rows]) fp32.
    dead: None, or bool [n_rows] -- the rows the forward gave a uniform softmax over all n_cols columns (the dead rows
    of the adjacency it masked with, quantised or not); their softmax row sum is G[r] . mean(Wh) (SG.py:884-1126)."""
    _dev2d(G, "G")
    _dev2d(Wh, "Wh")
    if G.dtype != torch.float32 or Wh.dtype != torch.float32 or E.dtype != torch.float32 or S.dtype != torch.float32:
        raise TypeError("gat_backward_edges works on float32 E, S, G, Wh (the reference's backward is fp32)")
    if Wh.shape[0] != adj.n_cols or G.shape != (adj.n_rows, Wh.shape[1]):
        raise ValueError("G must be [adj.n_rows, F] and Wh [adj.n_cols, F]")
    dead_rs, Wh = _backward_edge_operands(adj, G, Wh, dead)
    sg = torch.empty(adj.nnz, dtype=torch.float32, device=G.device)
    g1 = torch.empty(adj.n_rows, dtype=torch.float32, device=G.device)
    check(lib.sgx_gat_backward_edges(dtype_code(adj.val.dtype), adj.n_rows, adj.n_cols, Wh.shape[1], float(alpha),
                                     _ptr(adj.rowptr), _ptr(adj.col), _ptr(adj.val), _ptr(E.contiguous()), _ptr(S.contiguous()),
                                     _ptr(G), G.stride(0), _ptr(Wh), Wh.stride(0), _ptr(dead), _ptr(dead_rs), _ptr(sg),
                                     _ptr(g1), _stream()),
          "sgx_gat_backward_edges")
    return sg, g1


def gat_edge_outputs(adj, stats, alpha=0.2, dead_weight=0.0):
    """(E, S) fp32 [nnz] (heads > 1: [nnz, heads]) formed from the statistics of a forward that did not write them
    (sgx_gat_edge_outputs).  dead_weight: S on the stored entries of a row without a live entry -- the forward's dead-row
    rule: 1 / n_cols (mean fill), 1 / n_nodes (fill_row) or 0."""
    es_shape = (adj.nnz,) if stats.heads == 1 else (adj.nnz, stats.heads)
    E = torch.empty(es_shape, dtype=torch.float32, device=adj.val.device)
    S = torch.empty(es_shape, dtype=torch.float32, device=adj.val.device)
    st = stats.struct()
    check(lib.sgx_gat_edge_outputs(dtype_code(adj.val.dtype), adj.n_rows, adj.n_cols, stats.heads, float(alpha), _ptr(adj.rowptr),
                                   _ptr(adj.col), _ptr(adj.val), ctypes.byref(st), float(dead_weight), _ptr(E), _ptr(S),
                                   _stream()), "sgx_gat_edge_outputs")
    return E, S


def gat_backward_edges_stats(adj, stats, G, Wh, alpha=0.2, dead=None, dead_weight=0.0, want_S=True):
    """gat_backward_edges from the statistics instead of E and S (sgx_gat_backward_edges_stats, one head): returns
    (sg [nnz], g1 [n_rows], S [nnz] or None) -- S is the attention matrix's values, formed on the way for the caller's next
    product, not something the forward had to keep.  dead as in gat_backward_edges; dead_weight as in gat_edge_outputs."""
    _dev2d(G, "G")
    _dev2d(Wh, "Wh")
    if G.dtype != torch.float32 or Wh.dtype != torch.float32:
        raise TypeError("gat_backward_edges_stats works on float32 G, Wh (the reference's backward is fp32)")
    if Wh.shape[0] != adj.n_cols or G.shape != (adj.n_rows, Wh.shape[1]):
        raise ValueError("G must be [adj.n_rows, F] and Wh [adj.n_cols, F]")
    if stats.heads != 1:
        raise ValueError("the backward edge pass is single-head")
    dead_rs, Wh = _backward_edge_operands(adj, G, Wh, dead)
    sg = torch.empty(adj.nnz, dtype=torch.float32, device=G.device)
    g1 = torch.empty(adj.n_rows, dtype=torch.float32, device=G.device)
    S = torch.empty(adj.nnz, dtype=torch.float32, device=G.device) if want_S else None
    st = stats.struct()
    check(lib.sgx_gat_backward_edges_stats(dtype_code(adj.val.dtype), adj.n_rows, adj.n_cols, Wh.shape[1], 1, float(alpha),
                                           _ptr(adj.rowptr), _ptr(adj.col), _ptr(adj.val), ctypes.byref(st), float(dead_weight),
                                           _ptr(G), G.stride(0), _ptr(Wh), Wh.stride(0), _ptr(dead), _ptr(dead_rs), _ptr(sg),
                                           _ptr(g1), _ptr(S), _stream()), "sgx_gat_backward_edges_stats")
    return sg, g1, S


def gat_attention_grad(adj, sg, g1, Wh, schedule=None):
    """[Wh^T g1 ; Wh^T colsum(sg)] fp32 [2 F] from the edge pass's outputs, gathered over the stored entries in row order
    (sgx_gat_attention_grad): no transposed pattern; the same bits on every run.
    schedule="flat", or a matrix that carries the fact (Csr.with_facts(flat=True)): by stored entries
    (sgx_gat_attention_grad_flat) -- a hub row is spread over the chunks its entries fall in, the grid is a function of the
    entries adj.col holds (a capacity: the matrix's own end is read from rowptr on the device), and the result has the same
    bits at every capacity."""
    if schedule not in (None, "flat"):
        raise ValueError(f"schedule must be None or 'flat', not {schedule!r}")
    _dev2d(Wh, "Wh")
    if sg.dtype != torch.float32 or g1.dtype != torch.float32 or Wh.dtype != torch.float32:
        raise TypeError("gat_attention_grad works on float32 sg, g1, Wh")
    if Wh.shape[0] != adj.n_cols or adj.n_rows > adj.n_cols or g1.numel() != adj.n_rows or sg.numel() < adj.nnz:
        raise ValueError("Wh must be [adj.n_cols, F], g1 [adj.n_rows], sg [nnz], n_rows <= n_cols")
    F = Wh.shape[1]
    out = torch.empty(2 * F, dtype=torch.float32, device=Wh.device)
    if schedule == "flat" or adj._flat:
        nbytes = lib.sgx_gat_attention_grad_flat_workspace_bytes(adj.nnz, adj.n_rows, F)
        ws = _workspace(Wh.device, nbytes)
        check(lib.sgx_gat_attention_grad_flat(adj.n_rows, adj.n_cols, F, adj.nnz, _ptr(adj.rowptr), _ptr(adj.col), _ptr(sg), _ptr(g1),
                                              _ptr(Wh), Wh.stride(0), _ptr(out), _ptr(ws), ws.numel(), _stream()),
              "sgx_gat_attention_grad_flat")
        return out
    nbytes = lib.sgx_gat_attention_grad_workspace_bytes(adj.n_rows, F)
    ws = _workspace(Wh.device, nbytes)
    check(lib.sgx_gat_attention_grad(adj.n_rows, adj.n_cols, F, _ptr(adj.rowptr), _ptr(adj.col), _ptr(sg), _ptr(g1), _ptr(Wh),
                                     Wh.stride(0), _ptr(out), _ptr(ws), ws.numel(), _stream()), "sgx_gat_attention_grad")
    return out


def feature_csr32(x):
    """The fp32 CSR of a feature tensor and of its transpose, each built once per tensor (cached on it, as the forward's
    fea_csr is): what the one-call backward reads in gemm_mode 0 instead of a dense X.  Where the tensor already carries
    a flat-marked feature CSR of another element type (the forward's), the fact goes along: the pair built here is
    flat-marked too and wants no plan (the transpose of a flat-marked matrix is flat-marked).  That build is reached only off
    the loader path -- a caller who marked the forward's feature CSR by hand: it goes through a dense tensor and
    synchronises, and the pair carries no longest-row fact.  NeighborLoader(schedule="flat", transposed=True) delivers both
    entries itself, and nothing is built here."""
    def build():
        d = x.detach()
        Xc = Csr.from_dense(d if d.layout == torch.strided else d.to_dense(), torch.float32)       # (as the forward builds it)
        seen = [recorded(x, ("fea_csr", dt)) for dt in (torch.float16, torch.float32)]
        return Xc.with_facts(flat=True) if any(c is not None and c._flat for c in seen) else Xc

    Xc = cached_on(x, ("fea_csr", torch.float32), build)
    return Xc, cached_on(x, ("fea_csr_t", torch.float32), lambda: csr_transpose(Xc))


def layer_backward(adj, X, W, G, gat=False, gemm_mode=1, alpha=0.2, E=None, S=None, stats=None, dead_weight=0.0, dead=None,
                   mask=None, want_grad_input=True, schedule=None, _schedule_query=False):
    """The SGRACE layer's backward in one call (sgx_layer_backward): -> (grad_input [n, M] or None, grad_weights [M, P],
    grad_attention [2 P] or None), fp32.  adj: the forward's adjacency (GCN: its values are P); X: the layer's input -- a
    dense fp16|fp32 tensor (gemm_mode 1) or, gemm_mode 0, the feature tensor whose CSRs feature_csr32 caches (or that pair
    itself): never made dense; W [M, P] fp32; G = grad_output [n, P] fp32.  GAT: E and S, or stats with dead_weight; dead (bool [n]) the
    forward's dead rows; mask: the Csr whose values the edge pass masks with (default adj).  want_grad_input False: that
    product is not launched.
    schedule=None: each of the adjacency, the feature CSR and X^T that carries the entry-split fact (Csr.with_facts(flat=
    True)) has its products run on that schedule (sgx_layer_grad_desc.schedule_adj / _fea / _xt = SGX_SCHEDULE_FLAT at the
    entries its col holds, a capacity): no plan is built for it and nothing is read back, so the call records and replays
    at any fan-out.  "flat": all three, marked or not; "rows": none of them -- a flat-marked matrix runs by rows without a
    plan, as the layer does where its forward did not take the entry-split route."""
    if schedule not in (None, "flat", "rows"):
        raise ValueError(f"schedule must be None, 'flat' or 'rows', not {schedule!r}")
    is_flat = lambda m: schedule == "flat" or (schedule is None and m._flat)
    _dev2d(G, "G")
    _dev(W, "W")
    if G.dtype != torch.float32 or W.dtype != torch.float32:
        raise TypeError("the backward runs in float32: G and W must be float32")
    n, (M, P) = adj.n_rows, W.shape
    if adj.n_cols != n or G.shape != (n, P):
        raise ValueError("the adjacency must be square and G [n, P]")
    d = _lib.LayerGradDesc()
    d.gat_mode, d.gemm_mode, d.N_adj, d.M_adj, d.M_fea, d.P_w = int(bool(gat)), int(gemm_mode), n, n, M, P
    d.gat_heads, d.alpha, d.nnz_adj = 1, float(alpha), adj.nnz
    vals = (mask if (gat and mask is not None) else adj).val
    d.dtype_adj = dtype_code(vals.dtype)
    d.rowPtr_adj, d.columnIndex_adj, d.values_adj = adj.rowptr.data_ptr(), adj.col.data_ptr(), vals.data_ptr()
    keep = [vals]
    if is_flat(adj):
        d.schedule_adj = _lib.SGX_SCHEDULE_FLAT                # (nnz_adj above: what adj.col holds)
    else:
        plan = adj.plan if adj.wants_plan else None
        d.plan_adj = plan.handle if plan is not None else None
    if gemm_mode == 1:
        _dev2d(X, "X")
        if X.shape != (n, M):
            raise ValueError("X must be [n, M]")
        d.dtype_x, d.X, d.ldx = dtype_code(X.dtype), X.data_ptr(), X.stride(0)
    else:
        Xc, Xt = X if isinstance(X, tuple) else feature_csr32(X)
        if (Xc.n_rows, Xc.n_cols) != (n, M):
            raise ValueError("X must be [n, M]")
        d.dtype_x = SGX_F32
        d.rowPtr_fea, d.columnIndex_fea, d.values_fea = Xc.rowptr.data_ptr(), Xc.col.data_ptr(), Xc.val.data_ptr()
        d.rowPtr_xt, d.columnIndex_xt, d.values_xt = Xt.rowptr.data_ptr(), Xt.col.data_ptr(), Xt.val.data_ptr()
        if is_flat(Xc):
            d.schedule_fea, d.nnz_fea = _lib.SGX_SCHEDULE_FLAT, Xc.nnz
        else:
            d.plan_fea = Xc.plan.handle if Xc.wants_plan else None
        if is_flat(Xt):
            d.schedule_xt, d.nnz_xt = _lib.SGX_SCHEDULE_FLAT, Xt.nnz
        else:
            d.plan_xt = Xt.plan.handle if Xt.wants_plan else None
        keep += [Xc, Xt]
    d.W, d.G, d.ldg = W.data_ptr(), G.data_ptr(), G.stride(0)
    grad_attention = None
    if gat:
        if stats is not None:
            st = stats.struct()
            d.stats, d.dead_weight = ctypes.pointer(st), float(dead_weight)
        else:
            E, S = _dev(E, "E"), _dev(S, "S")
            if E.dtype != torch.float32 or S.dtype != torch.float32:
                raise TypeError("E and S are float32")
            d.E, d.S = E.data_ptr(), S.data_ptr()
        if dead is not None:
            _dev(dead, "dead")
            if dead.dtype != torch.bool or dead.shape != (n,):
                raise ValueError("dead must be a bool [n] tensor")
            d.dead = dead.data_ptr()                      # (a bool tensor is one byte of 0 / 1 per element)
        grad_attention = torch.empty(2 * P, dtype=torch.float32, device=G.device)
        d.grad_attention = grad_attention.data_ptr()
    grad_weights = torch.empty((M, P), dtype=torch.float32, device=G.device)
    d.grad_weights = grad_weights.data_ptr()
    grad_input = None
    if want_grad_input:
        grad_input = torch.empty((n, table_pitch(M, 4)), dtype=torch.float32, device=G.device)
        d.grad_input, d.ld_gi = grad_input.data_ptr(), grad_input.stride(0)
    if _schedule_query:
        route = lib.sgx_layer_backward_schedule(ctypes.byref(d))
        if route < 0:
            check(int(route), "sgx_layer_backward_schedule")
        return route
    nbytes = lib.sgx_layer_backward_workspace_bytes(ctypes.byref(d))
    ws = _workspace(G.device, nbytes)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    check(lib.sgx_layer_backward(ctypes.byref(d), _stream()), "sgx_layer_backward")
    return (None if grad_input is None else grad_input[:, :M]), grad_weights, grad_attention


def layer_backward_schedule(adj, X, W, G, **kwargs):
    """Which schedules layer_backward(adj, X, W, G, **kwargs) takes, from the very descriptor it builds
    (sgx_layer_backward_schedule; no launch): bit 0 the adjacency's products, bit 1 Wh = X . W, bit 2 X^T . pg entry-split."""
    return layer_backward(adj, X, W, G, _schedule_query=True, **kwargs)


def readout_mean_linear(x, graph_ptr, weight=None, bias=None, want_pooled=False):
    """global_mean_pool over contiguous graphs + Linear head in one launch (sgx_readout_mean_linear).
    x [n, F] fp16|fp32, graph_ptr int32 [n_graphs+1], weight [C, F] fp32, bias [C] fp32."""
    _dev2d(x, "x")
    _dev(graph_ptr, "graph_ptr")
    n_graphs, F = graph_ptr.numel() - 1, x.shape[1]
    C = 0 if weight is None else weight.shape[0]
    pooled = torch.empty((n_graphs, F), dtype=torch.float32, device=x.device) if (want_pooled or weight is None) else None
    logits = torch.empty((n_graphs, C), dtype=torch.float32, device=x.device) if weight is not None else None
    w = None if weight is None else _dev(weight.detach().float().contiguous(), "weight")
    b = None if bias is None else _dev(bias.detach().float().contiguous(), "bias")
    check(lib.sgx_readout_mean_linear(dtype_code(x.dtype), n_graphs, F, C, _ptr(x), x.stride(0), _ptr(graph_ptr),
                                      _ptr(w), _ptr(b), _ptr(pooled), _ptr(logits), _stream()), "sgx_readout_mean_linear")
    if weight is None:
        return pooled
    return (logits, pooled) if want_pooled else logits


def readout_mean_backward(grad_pooled, graph_ptr, n_rows, dtype, covers_all_rows=False):
    """grad of the rows a global_mean_pool read (sgx_readout_mean_backward): grad_pooled fp32 [n_graphs, F] -> [n_rows, F]
    in `dtype`, each row its graph's gradient over the graph's size; rows of no graph get 0 (covers_all_rows: the caller
    knows there are none, e.g. graph_ptr_of(batch), and the result needs no clearing first)."""
    _dev2d(grad_pooled, "grad_pooled")
    _dev(graph_ptr, "graph_ptr")
    g = grad_pooled.float().contiguous()
    out = (torch.empty if covers_all_rows else torch.zeros)((n_rows, g.shape[1]), dtype=dtype, device=g.device)
    check(lib.sgx_readout_mean_backward(dtype_code(dtype), graph_ptr.numel() - 1, g.shape[1], _ptr(g), _ptr(graph_ptr), _ptr(out),
                                        out.stride(0), _stream()), "sgx_readout_mean_backward")
    return out


class ReadoutMean(torch.autograd.Function):
    """global_mean_pool over contiguous graphs as one launch each way (MOL cell 18's pooling inside the training step):
    forward = sgx_readout_mean_linear without a head (fp32 means in row order), backward = sgx_readout_mean_backward."""

    @staticmethod
    def forward(ctx, x, graph_ptr, covers_all_rows=False):
        ctx.save_for_backward(graph_ptr)
        ctx.about_x = (x.shape[0], x.dtype, bool(covers_all_rows))
        return readout_mean_linear(x.contiguous(), graph_ptr)

    @staticmethod
    def backward(ctx, grad):
        (graph_ptr,) = ctx.saved_tensors
        n, dtype, covers = ctx.about_x
        return readout_mean_backward(grad, graph_ptr, n, dtype, covers), None, None


def graph_ptr_of(batch):
    """graph_ptr [n_graphs + 1] int32 of a sorted PyG `batch` vector, kept on the tensor (an epoch loop passes the same
    batch every step); None when `batch` is not sorted, so that its graphs are not row segments (checked once per
    tensor, one device->host sync)."""
    def build():
        if batch.numel() > 1 and not bool((batch[1:] >= batch[:-1]).all().item()):
            return None
        counts = torch.bincount(batch)
        ptr = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=batch.device)
        ptr[1:] = torch.cumsum(counts, 0)
        return ptr
    return cached_on(batch, ("graph_ptr",), build)


def relu_mask_backward_(out, grad):
    """grad[out == 0] = 0 in place (RPYNQ.backward, MOL cell 16)."""
    _dev(out, "out")
    _dev(grad, "grad")
    check(lib.sgx_relu_mask_backward(dtype_code(out.dtype), _ptr(out), dtype_code(grad.dtype), _ptr(grad),
                                     out.numel(), _stream()), "sgx_relu_mask_backward")
    return grad


# ---- neighbour sampling (sgx_sample_neighbors): the NeighborLoader batches of demo_sgrace.py:112-125 ----------------
SAMPLE_SENTINEL = 0x7FFFFFFF
SAMPLE_WIDE_MAX = lib.sgx_sample_wide_max()     # the largest fan-out whose subset a whole wavefront builds in LDS
_node_maps = {}


def sample_form(fanout):
    """Which form of the subset step a hop with this fan-out runs on rows over the fan-out (sgx_sample_form): 0 = -1,
    every position; 1 = up to 64, in registers; 2 = 65 .. SAMPLE_WIDE_MAX, in LDS; 3 = above, one lane.  The same bits
    come out of every form.  ValueError below -1.  No device needed."""
    form = lib.sgx_sample_form(int(fanout))
    if form < 0:
        raise ValueError(f"sample_form: fan-out {fanout} is below -1")
    return form


def _node_map(device, n_nodes):
    """The sampler's node -> local id map, one per (device, stream), kept at the sentinel between calls."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    m = _node_maps.get(key)
    if m is None or m.numel() < n_nodes:
        m = torch.full((max(int(n_nodes), 1),), SAMPLE_SENTINEL, dtype=torch.int32, device=device)
        _node_maps[key] = m
    return m


def _fan_array(fanouts):
    """-> (the fan-outs as a list of int, the same as the int32 array the C calls read)"""
    fan = [int(k) for k in fanouts]
    return fan, (ctypes.c_int32 * max(len(fan), 1))(*fan)


def _sampler_workspace(call, query, csr, B, fan, fan_c):
    """-> (workspace, max_nodes, max_edges): the scratch of one sampling call as `query` (an sgx_*_workspace_bytes) sizes
    it, and the sampler's bounds on the batch's nodes and edges.  ValueError naming `call` where the query refuses."""
    max_nodes, max_edges = ctypes.c_int64(0), ctypes.c_int64(0)
    nbytes = query(csr.n_rows, csr.nnz, B, len(fan), fan_c, ctypes.byref(max_nodes), ctypes.byref(max_edges))
    if nbytes == 0:
        raise ValueError(f"{call}: bad arguments (n_nodes {csr.n_rows}, nnz {csr.nnz}, batch {B}, fanouts {fan}): "
                         "fan-outs must be >= -1, 1 to 64 hops, batch <= n_nodes")
    return _workspace(csr.rowptr.device, nbytes), max_nodes.value, max_edges.value


def _check_sample(status, node_map, call):
    """check() of an eager sampling call's status, with the map put back first where the library left it used."""
    if status not in (0, _lib.SGX_ERR_SEEDS):
        node_map.fill_(SAMPLE_SENTINEL)                 # (sgx.h: the map is restored on success and on SGX_ERR_SEEDS only)
    check(status, call)


class Sample:
    """One sampled mini-batch (include/sgx.h, "neighbour sampling"): n_id (global ids, seeds first), adj (Csr over the
    local nodes: row i = the sampled in-neighbours of local node i), edge_pos (position of every sampled edge in the
    input CSR), batch_size, and the node / edge counts after each hop (num_sampled_* as PyG counts them: per hop)."""

    def __init__(self, n_id, adj, edge_pos, batch_size, hop_nodes, hop_edges):
        self.n_id, self.adj, self.edge_pos, self.batch_size = n_id, adj, edge_pos, batch_size
        self.hop_nodes, self.hop_edges = list(hop_nodes), list(hop_edges)

    @property
    def num_sampled_nodes(self):
        h = self.hop_nodes
        return [h[0]] + [h[i + 1] - h[i] for i in range(len(h) - 1)]

    @property
    def num_sampled_edges(self):
        h = self.hop_edges
        return [h[i + 1] - h[i] for i in range(len(h) - 1)]


def sample_neighbors(csr, seeds, fanouts, seed=0, step=0, gather_values=False):
    """Neighbour sample of `seeds` (int32 or int64 global ids on the device, unique) over `csr` (row v = the in-edges
    of v), one fan-out per hop (-1 = every neighbour), by the rule of include/sgx.h: the same bits for the same
    (graph, seeds, fanouts, seed, step).  adj holds fp32 ones, or the sampled entries of csr.val with gather_values.
    One stream synchronisation per call."""
    _dev(seeds, "seeds")
    dev = csr.rowptr.device
    seeds = seeds.to(torch.int32).contiguous()
    B, n = seeds.numel(), csr.n_rows
    fan, fan_c = _fan_array(fanouts)
    H = len(fan)
    ws, mn, me = _sampler_workspace("sample_neighbors", lib.sgx_sample_workspace_bytes, csr, B, fan, fan_c)
    i32 = lambda k: torch.empty(max(int(k), 1), dtype=torch.int32, device=dev)
    n_id, rowptr, col, pos = i32(mn), i32(mn + 1), i32(me), i32(me)
    hop_nodes, hop_edges = (ctypes.c_int64 * (H + 1))(), (ctypes.c_int64 * (H + 1))()
    node_map = _node_map(dev, n)
    status = lib.sgx_sample_neighbors(_ptr(csr.rowptr), _ptr(csr.col), n, csr.nnz, _ptr(seeds) if B else None, B, H, fan_c,
                                      int(seed) & (2**64 - 1), int(step) & (2**64 - 1), _ptr(node_map), _ptr(n_id),
                                      _ptr(rowptr), _ptr(col), _ptr(pos), mn, me, hop_nodes, hop_edges, _ptr(ws), ws.numel(),
                                      _stream())
    _check_sample(status, node_map, "sgx_sample_neighbors")
    N, E = hop_nodes[H], hop_edges[H]
    val = csr.val[pos[:E].long()] if gather_values else torch.ones(E, dtype=torch.float32, device=dev)
    adj = Csr(rowptr[:N + 1], col[:E], val, N)
    return Sample(n_id[:N], adj, pos[:E], B, hop_nodes[:], hop_edges[:])


class NodeSample(Sample):
    """A Sample prepared for the layers on the device (sample_node_batch): besides the sample, adj_norm -- the Csr of
    sym_norm2 over adj in the requested dtype, with its dead-row mask, flag and longest row recorded --, edge_index /
    edge_index_agg (int64 [2, E]: PyG's orientation / row 0 the aggregating node), fea (the feature Csr of the rows
    n_id, or None), y and masks (gathered at n_id, or None / empty)."""


def feature_csr(x):
    """The fp32 CSR of a dense feature matrix with its longest row recorded: what sample_node_batch gathers batches'
    feature CSRs from.  Synchronises (once per dataset)."""
    fea = Csr.from_dense(x.float())
    longest = int((fea.rowptr[1:] - fea.rowptr[:-1]).max().item()) if fea.n_rows else 0
    return fea.with_facts(max_row=longest)


def _adj_quant_key(qc):
    """The key Csr.quantized files a quantised adjacency under: the constants the adjacency's quantiser reads."""
    return (qc.w_qbits, qc.a_s, qc.a_z)


def _adj_quant_sets(quant):
    """{_adj_quant_key: constants} of the quantised adjacencies a batch for `quant` carries, in order: one set per distinct
    key of quant and quant.second_layer() (the demo's two layers share the adjacency's constants); {} without quant."""
    return {} if quant is None else {_adj_quant_key(qc): qc for qc in (quant, quant.second_layer())}


class PaddedNodeSample(NodeSample):
    """A NodeSample at a fixed capacity (sample_node_batch(pad=); include/sgx.h, "padded node batches"): every tensor has
    its capacity size in every batch, the live rows and entries first and filler rows behind (n_id = -1).  The live
    counts stay on the device -- `counts`, int32: n, edges, adjacency entries, feature entries, then the node and the edge
    count after every hop -- so hop_nodes / hop_edges are empty and num_sampled_nodes / num_sampled_edges None.  adj is
    None: the sampled CSR has spare entries behind its last row (its raw arrays are out_rowptr, out_col and edge_pos,
    -1 past the live edges); adj_norm and fea are exact CSRs.  The tensors are views of the NodePadBuffers the call wrote:
    valid until the next batch is drawn into them."""

    num_sampled_nodes = num_sampled_edges = None


class NodePadCapacity:
    """The fixed sizes of a padded node batch (node_pad_capacity): n_rows (N), nnz_norm (C_a), nnz_fea (C_f), n_edges (E),
    the sampler's bounds max_nodes / max_edges they come from, batch_size, fanouts, whether a feature CSR was counted, and
    max_row = max(max(fanouts) + 1, 64), the bound on the longest row of the normalised adjacency."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def node_pad_capacity(csr, batch_size, fanouts, features=None):
    """The capacity every batch of `batch_size` seeds sampled from `csr` with `fanouts` fits (sgx_node_batch_pad_capacity;
    rule and proof in include/sgx.h): host arithmetic, computed once per (graph, batch, fanouts, feature CSR).  features:
    the feature_csr of the graph's x, or None; its per-row entry counts are read back once here."""
    fan, fan_c = _fan_array(fanouts)
    H = len(fan)
    if any(k < 0 for k in fan):
        raise ValueError("node_pad_capacity: a fan-out of -1 leaves a row unbounded; padded batches need fan-outs >= 0")
    rows = None
    if features is not None:
        rows = (features.rowptr[1:] - features.rowptr[:-1]).to(torch.int32).cpu().contiguous()
    p = _lib.NodeBatchPad()
    check(lib.sgx_node_batch_pad_capacity(csr.n_rows, csr.nnz, int(batch_size), H, fan_c,
                                          _ptr(rows), ctypes.byref(p)), "sgx_node_batch_pad_capacity")
    mn, me = ctypes.c_int64(0), ctypes.c_int64(0)
    lib.sgx_node_batch_workspace_bytes(csr.n_rows, csr.nnz, int(batch_size), H, fan_c, ctypes.byref(mn), ctypes.byref(me))
    return NodePadCapacity(n_rows=p.n_rows, nnz_norm=p.nnz_norm, nnz_fea=p.nnz_fea, n_edges=p.n_edges, max_nodes=mn.value,
                           max_edges=me.value, batch_size=int(batch_size), fanouts=tuple(fan), features=features is not None,
                           max_row=max(max(fan) + 1, 64))


class NodePadBuffers:
    """The output buffers of padded node batches of one capacity, written again by every sample_node_batch(pad=, out=):
    what a recorded step reads at fixed addresses.  Also the sampler's node map (kept at the sentinel between calls), the
    OR-ed status word and the live counts.  n_id starts at -1, so no gather by it ever leaves its source.  n_quant: the
    number of constant sets of a quantised padded batch (sample_node_batch(pad=, quant=)); `quant` then holds (q_val [C_a]
    fp32, q_dead [N] bool, q_lean [C_a] fp32) per set.  worst_case: the same arrays for one unpadded batch."""

    def __init__(self, cap, n_nodes, dtype, device, n_feat=None, y=False, n_masks=0, n_quant=0):
        new = lambda k, dt, v=0: torch.full((max(int(k), 1),), v, dtype=dt, device=device)
        self.capacity, self.dtype = cap, dtype
        self._outputs(new, cap.n_rows, cap.n_edges, cap.nnz_norm, cap.nnz_fea if cap.features else None, dtype, y, n_masks, n_quant)
        if cap.features:
            self.n_feat = int(n_feat)
        self.max_nodes, self.max_edges = cap.max_nodes, cap.max_edges
        self.node_map = new(n_nodes, torch.int32, SAMPLE_SENTINEL)
        self.status = new(1, torch.int32)
        self.counts = new(4 + 2 * (len(cap.fanouts) + 1), torch.int32)

    def _outputs(self, new, N, E, Ca, Cf, dtype, y, n_masks, n_quant):
        """Every output array of a batch of up to N nodes, E edges, Ca adjacency and Cf feature entries (None: no feature
        CSR), each from new(size, dtype[, fill])."""
        self.n_id, self.rowptr, self.col, self.pos = new(N, torch.int32, -1), new(N + 1, torch.int32), new(E, torch.int32, -1), new(E, torch.int32, -1)
        self.n_rowptr, self.n_col, self.n_val = new(N + 1, torch.int32), new(Ca, torch.int32), new(Ca, dtype)
        self.dead = new(N, torch.bool, False)
        self.ei, self.ei_agg = new(2 * E, torch.int64, -1), new(2 * E, torch.int64, -1)
        self.f_rowptr = self.f_col = self.f_val = None
        if Cf is not None:
            self.f_rowptr, self.f_col, self.f_val = new(N + 1, torch.int32), new(Cf, torch.int32), new(Cf, dtype)
        self.y = new(N, torch.int64) if y else None
        self.masks = [new(N, torch.bool, False) for _ in range(n_masks)]
        self.quant = [(new(Ca, torch.float32), new(N, torch.bool, False), new(Ca, torch.float32)) for _ in range(int(n_quant))]

    @classmethod
    def worst_case(cls, max_nodes, max_edges, dtype, device, fea_capacity, y, n_masks, n_quant, node_map):
        """The buffers of ONE unpadded batch at the sampler's bounds, unfilled (the kernels write all that is read), over the
        stream's shared node map: what sample_node_batch without pad= draws into and returns views of."""
        self = object.__new__(cls)
        empty = lambda k, dt, v=None: torch.empty(max(int(k), 1), dtype=dt, device=device)
        self._outputs(empty, max_nodes, max_edges, max_edges + max_nodes, fea_capacity, dtype, y, n_masks, n_quant)
        self.max_nodes, self.max_edges, self.node_map = max_nodes, max_edges, node_map
        return self


def _check_node_batch(csr, seeds, dtype, edge_weight, features, y, masks, quant):
    """The argument checks of sample_node_batch, padded or not -> (seeds as int32, masks as a list)."""
    _dev(seeds, "seeds")
    n = csr.n_rows
    if quant is not None and dtype != torch.float32:
        raise ValueError("sample_node_batch: quant needs dtype=torch.float32 (the quantised layer works on float32 buffers)")
    masks = list(masks)
    if len(masks) > 3:
        raise ValueError("sample_node_batch gathers up to three masks")
    if features is not None and (features.val.dtype != torch.float32 or features.n_rows != n or features._max_row is None):
        raise ValueError("features must be the feature_csr of the graph's x (fp32 values, one row per node)")
    optional = [(edge_weight, "edge_weight", torch.float32, csr.nnz, "edge_weight must be float32 [csr.nnz]"),
                (y, "y", torch.int64, n, "y must be int64 [n_nodes]")]
    for t, name, dt, size, what in ([c for c in optional if c[0] is not None]
                                    + [(m, "mask", torch.bool, n, "masks must be bool [n_nodes]") for m in masks]):
        _dev(t, name)
        if t.dtype != dt or t.numel() != size:
            raise ValueError(what)
    return seeds.to(torch.int32).contiguous(), masks


def _node_batch_desc(csr, seeds, fan, fan_c, seed, dtype, edge_weight, fill, features, y, masks, out, ws):
    """struct sgx_node_batch of checked arguments, writing into `out` (a NodePadBuffers of either kind).  The caller adds
    what its mode alone has: the host step, hop_nodes / hop_edges and fea_capacity, or the NodeBatchPad."""
    b = _lib.NodeBatch()
    B = seeds.numel()
    b.rowPtr, b.columnIndex, b.n_nodes, b.nnz = csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.n_rows, csr.nnz
    b.seeds, b.batch, b.n_hops, b.fanouts = (seeds.data_ptr() if B else None), B, len(fan), fan_c
    b.dtype, b.seed, b.fill = dtype_code(dtype), int(seed) & (2**64 - 1), float(fill)
    b.node_map, b.n_id, b.out_rowPtr, b.out_col, b.edge_pos = (out.node_map.data_ptr(), out.n_id.data_ptr(), out.rowptr.data_ptr(),
                                                               out.col.data_ptr(), out.pos.data_ptr())
    b.max_nodes, b.max_edges = out.max_nodes, out.max_edges
    if edge_weight is not None:
        b.edge_weight = edge_weight.data_ptr()
    b.rowPtr_norm, b.columnIndex_norm, b.values_norm = out.n_rowptr.data_ptr(), out.n_col.data_ptr(), out.n_val.data_ptr()
    b.dead_row, b.edge_index, b.edge_index_agg = out.dead.data_ptr(), out.ei.data_ptr(), out.ei_agg.data_ptr()
    if features is not None:
        b.rowPtr_x, b.columnIndex_x, b.values_x = features.rowptr.data_ptr(), features.col.data_ptr(), features.val.data_ptr()
        b.rowPtr_fea, b.columnIndex_fea, b.values_fea = out.f_rowptr.data_ptr(), out.f_col.data_ptr(), out.f_val.data_ptr()
    if y is not None:
        b.y, b.y_out = y.data_ptr(), out.y.data_ptr()
    for k, m in enumerate(masks):
        b.mask[k], b.mask_out[k] = m.data_ptr(), out.masks[k].data_ptr()
    b.workspace, b.workspace_bytes = ws.data_ptr(), ws.numel()
    return b


def _node_batch_quant_desc(sets, out):
    """struct sgx_node_batch_quant of the constant sets `sets` (_adj_quant_sets), writing into out.quant; None without sets."""
    if not sets:
        return None
    q = _lib.NodeBatchQuant()
    q.n_sets, q.qbits = len(sets), int(next(iter(sets.values())).w_qbits)
    for k, (qc, (q_val, q_dead, q_lean)) in enumerate(zip(sets.values(), out.quant)):
        q.inv_scale_adj[k], q.zero_adj[k] = float(1 / qc.a_s), float(qc.a_z)
        q.values_q[k], q.dead_row_q[k], q.values_lean[k] = q_val.data_ptr(), q_dead.data_ptr(), q_lean.data_ptr()
    return q


def _node_batch_call(b, p, q):
    """The one of the four sgx_node_batch_sample* entries that takes these descriptors (p the NodeBatchPad, q the
    NodeBatchQuant; None: the entry without) on the current stream -> (status, the entry's name)."""
    name = "sgx_node_batch_sample" + ("_padded" if p is not None else "") + ("_quant" if q is not None else "")
    return getattr(lib, name)(*[ctypes.byref(d) for d in (b, p, q) if d is not None], _stream()), name


def _wrap_node_batch(s, out, sets, features, N, E, nnz_norm, nnz_fea, has_dead_rows, has_dead_rows_q, max_row, fea_max_row):
    """Fills the NodeSample `s` with what a batch call wrote into `out`, as views of N nodes, E edges, nnz_norm adjacency and
    nnz_fea feature entries with the given facts (has_dead_rows_q: one per set of `sets`).  Every array is cut to its
    count: an empty Csr keeps one-element stand-ins for col and val, which must not pass for an entry."""
    s.adj_norm = A = Csr(out.n_rowptr[:N + 1], out.n_col[:nnz_norm], out.n_val[:nnz_norm], N).with_facts(
        out.dead[:N], has_dead_rows, max_row)
    col = A.col if A.nnz else A.col[:0]                 # the quantised adjacencies share A's pattern, the tensors themselves
    for key, (q_val, q_dead, q_lean), dead_q in zip(sets, out.quant, has_dead_rows_q):
        Q = Csr(A.rowptr, col, q_val[:nnz_norm], N).with_facts(q_dead[:N], dead_q, max_row)
        Q._lean_values = Csr(A.rowptr, col, q_lean[:nnz_norm], N)
        A._quantized[key] = Q
    s.edge_index, s.edge_index_agg = out.ei[:2 * E].view(2, E), out.ei_agg[:2 * E].view(2, E)
    s.fea = None
    if features is not None:
        s.fea = Csr(out.f_rowptr[:N + 1], out.f_col[:nnz_fea], out.f_val[:nnz_fea], features.n_cols).with_facts(max_row=fea_max_row)
    s.y = None if out.y is None else out.y[:N]
    s.masks = [m[:N] for m in out.masks]
    return s


def _sample_node_batch_padded(csr, seeds, fan, fan_c, seed, step, fill, dtype, edge_weight, features, y, masks, sets, cap, out):
    """sample_node_batch(pad=cap) of checked arguments: sgx_node_batch_sample_padded -- with constant sets
    sgx_node_batch_sample_padded_quant -- into `out` (a NodePadBuffers; None: a fresh one).  Reads nothing back."""
    dev, n, B = csr.rowptr.device, csr.n_rows, seeds.numel()
    if tuple(fan) != cap.fanouts:
        raise ValueError("sample_node_batch: pad= was computed for other fan-outs")
    if B != cap.batch_size or cap.features != (features is not None):
        raise ValueError("sample_node_batch: pad= is the node_pad_capacity of this batch size, these fan-outs and these features")
    _dev(step, "step")
    if step.dtype != torch.int64 or step.numel() != 1:
        raise ValueError("sample_node_batch(pad=): step is a device int64 [1] tensor (the word a replay reads)")
    if out is None:
        out = NodePadBuffers(cap, n, dtype, dev, None if features is None else features.n_cols, y is not None, len(masks),
                             len(sets))
    if (out.capacity is not cap or out.dtype != dtype or (out.y is None) != (y is None) or len(out.masks) != len(masks)
            or len(out.quant) != len(sets)):
        raise ValueError("sample_node_batch: out= was built for another capacity, dtype, label, mask set or number of "
                         "quantiser constant sets")
    ws = _workspace(dev, lib.sgx_node_batch_workspace_bytes(n, csr.nnz, B, len(fan), fan_c, None, None))
    b = _node_batch_desc(csr, seeds, fan, fan_c, seed, dtype, edge_weight, fill, features, y, masks, out, ws)
    N, Ca, Cf, E = cap.n_rows, cap.nnz_norm, cap.nnz_fea, cap.n_edges
    p = _lib.NodeBatchPad()
    p.n_rows, p.nnz_norm, p.nnz_fea, p.n_edges = N, Ca, Cf, E
    p.step, p.status, p.counts = step.data_ptr(), out.status.data_ptr(), out.counts.data_ptr()
    check(*_node_batch_call(b, p, _node_batch_quant_desc(sets, out)))
    s = PaddedNodeSample(out.n_id[:N], None, out.pos[:E], B, [], [])
    s.buffers, s.counts, s.status = out, out.counts, out.status
    s.out_rowptr, s.out_col = out.rowptr[:N + 1], out.col[:E]
    # the capacity's constant facts: one kernel path for every batch, nothing read back
    return _wrap_node_batch(s, out, sets, features, N, E, Ca, Cf, True, [True] * len(sets), cap.max_row,
                            None if features is None else max(features._max_row, 64))


def sample_node_batch(csr, seeds, fanouts, seed=0, step=0, fill=0, dtype=torch.float32, edge_weight=None, features=None,
                      y=None, masks=(), quant=None, pad=None, out=None):
    """sample_neighbors plus, on the device right behind it and inside the same single synchronisation
    (sgx_node_batch_sample, rule in include/sgx.h): the normalised adjacency sym_norm2 gives for the sampled rows,
    the rows n_id of `features` (a feature_csr) as the batch's feature Csr, y[n_id] (int64) and each of up to three
    bool `masks` at n_id.  edge_weight: fp32 [csr.nnz] weights of the graph's edges (None = 1).  -> NodeSample.
    quant (a quant.QuantConstants, fp32 only): the batch is also ready for the quantised layers
    (sgx_node_batch_sample_quant, same single synchronisation): adj_norm.quantized(qc) for quant and for
    quant.second_layer() is delivered -- the values on the unsigned w_qbits grid with their dead-row mask, flag and
    longest row recorded, and the mask values of the lean GAT backward (sgrace._lean_mask) -- so that the layers launch no
    quantiser for the adjacency and read nothing back.
    pad (a node_pad_capacity of this batch size, fan-outs and features) with step a device int64 [1] tensor: the same
    batch at the capacity's fixed sizes (sgx_node_batch_sample_padded) -> PaddedNodeSample, written into `out` (the
    NodePadBuffers of an earlier call, at `.buffers` of what it returned; None: fresh ones).  The live prefix of every
    tensor holds the unpadded call's bits for the step the word holds; the facts are constants -- max_row =
    max(max(fanouts) + 1, 64), has_dead_rows = True with the exact mask -- and nothing is read from the device: no
    synchronisation, capturable.  Errors of the sample (repeated seeds) reach out.status, not an exception.
    pad with quant (sgx_node_batch_sample_padded_quant, fp32 only): the padded batch also carries adj_norm.quantized(qc)
    for quant and quant.second_layer() at capacity size -- the live prefix holds the unpadded quant= call's bits, a filler
    row fq(1) on its diagonal entry and fq(0) on its spare ones -- with the same constant facts (has_dead_rows = True with
    the exact quantised mask) and the lean mask values.  The constants must leave fq(1) > 0 and fq(0) == 0 (SgxError
    otherwise): a filler row is then not dead and its spare entries carry no weight.  out= holds one (values, mask, lean
    values) triple per distinct constant set; one built for another number of sets is refused."""
    fan, fan_c = _fan_array(fanouts)
    seeds, masks = _check_node_batch(csr, seeds, dtype, edge_weight, features, y, masks, quant)
    sets = _adj_quant_sets(quant)
    if pad is not None:
        return _sample_node_batch_padded(csr, seeds, fan, fan_c, seed, step, fill, dtype, edge_weight, features, y, masks, sets,
                                         pad, out)
    if out is not None:
        raise ValueError("sample_node_batch: out= needs pad=")
    dev, B, H = csr.rowptr.device, seeds.numel(), len(fan)
    ws, mn, me = _sampler_workspace("sample_node_batch", lib.sgx_node_batch_workspace_bytes, csr, B, fan, fan_c)
    fea_capacity = None if features is None else min(features.nnz, mn * features._max_row)
    out = NodePadBuffers.worst_case(mn, me, dtype, dev, fea_capacity, y is not None, len(masks), len(sets),
                                    _node_map(dev, csr.n_rows))
    b = _node_batch_desc(csr, seeds, fan, fan_c, seed, dtype, edge_weight, fill, features, y, masks, out, ws)
    b.step = int(step) & (2**64 - 1)
    hop_nodes, hop_edges = (ctypes.c_int64 * (H + 1))(), (ctypes.c_int64 * (H + 1))()
    b.hop_nodes, b.hop_edges = hop_nodes, hop_edges
    if features is not None:
        b.fea_capacity = fea_capacity
    q = _node_batch_quant_desc(sets, out)
    status, call = _node_batch_call(b, None, q)
    _check_sample(status, out.node_map, call)
    N, E = hop_nodes[H], hop_edges[H]                   # what the call read back, inside its one synchronisation
    adj = Csr(out.rowptr[:N + 1], out.col[:E], torch.ones(E, dtype=torch.float32, device=dev), N)
    s = NodeSample(out.n_id[:N], adj, out.pos[:E], B, hop_nodes[:], hop_edges[:])
    return _wrap_node_batch(s, out, sets, features, N, E, b.nnz_norm, b.nnz_fea, b.has_dead_rows, q.has_dead_rows_q if sets else (), b.max_row,
                            None if features is None else features._max_row)


# ---- a batch of small graphs through the whole GCN stack in one launch (sgx_stack_forward) ----------------------------
class BatchPlan:
    """Groups of whole graphs for sgx_stack_forward (sgx_batch_plan): graph_ptr and the adjacency are checked on the
    device to be block-diagonal (SgxError SGX_ERR_BLOCKS otherwise) and the graphs are cut into runs of at most `rows`
    rows, what the fused kernel keeps in LDS for layers up to max_width columns.  `fits` is False when a graph is larger
    than that; the stack then takes the chained kernels.  One stream synchronisation per plan.
    kind: _lib.SGX_BATCH_FORWARD, or SGX_BATCH_BACKWARD for the smaller row budget of sgx_stack_backward (such a plan
    serves the forward too)."""

    def __init__(self, adj, graph_ptr, max_width, kind=_lib.SGX_BATCH_FORWARD):
        _dev(graph_ptr, "graph_ptr")
        if graph_ptr.dtype != torch.int32:
            raise TypeError("graph_ptr must be int32")
        self.dtype = adj.val.dtype
        self.n_rows, self.n_graphs, self.max_width = adj.n_rows, graph_ptr.numel() - 1, int(max_width)
        self.kind = int(kind)
        self.trusted = False                   # (checked on the device; BatchPlan.known: True)
        h = ctypes.c_void_p()
        if self.kind == _lib.SGX_BATCH_FORWARD:
            check(lib.sgx_batch_plan_create(dtype_code(self.dtype), self.n_rows, self.n_graphs, _ptr(graph_ptr),
                                            _ptr(adj.rowptr), _ptr(adj.col), self.max_width, ctypes.byref(h), _stream()),
                  "sgx_batch_plan_create")
        else:
            check(lib.sgx_batch_plan_create_ex(dtype_code(self.dtype), self.n_rows, self.n_graphs, _ptr(graph_ptr),
                                               _ptr(adj.rowptr), _ptr(adj.col), self.max_width, self.kind, ctypes.byref(h),
                                               _stream()), "sgx_batch_plan_create_ex")
        self._h = h

    @classmethod
    def known(cls, graph_ptr, n_rows, dtype, max_graph, max_width, kind=_lib.SGX_BATCH_FORWARD):
        """The trusted plan (sgx_batch_plan_create_known) of a batch whose blocks the caller vouches for -- graph_ptr cuts
        its adjacency into diagonal blocks, the largest of max_graph rows -- as the collator's batches are: the plan
        BatchPlan gives on the same batch, without its device checks, read-back and stream synchronisation.  The
        group_graph table lives in a tensor this object keeps."""
        _dev(graph_ptr, "graph_ptr")
        if graph_ptr.dtype != torch.int32:
            raise TypeError("graph_ptr must be int32")
        self = cls.__new__(cls)
        self._h = None
        self.trusted = True
        self.dtype = dtype
        self.n_rows, self.n_graphs, self.max_width, self.kind = int(n_rows), graph_ptr.numel() - 1, int(max_width), int(kind)
        code = dtype_code(dtype)
        n = lib.sgx_batch_plan_group_count(code, self.n_rows, int(max_graph), self.max_width, self.kind)
        if n < 0:
            check(n, "sgx_batch_plan_group_count")
        self._group_graph = torch.empty(n + 1, dtype=torch.int32, device=graph_ptr.device) if n > 0 else None
        h = ctypes.c_void_p()
        check(lib.sgx_batch_plan_create_known(code, self.n_rows, self.n_graphs, _ptr(graph_ptr), int(max_graph), self.max_width,
                                              self.kind, _ptr(self._group_graph), ctypes.byref(h), _stream()),
              "sgx_batch_plan_create_known")
        self._h = h
        return self

    @staticmethod
    def cached(adj, graph_ptr, max_width, kind=_lib.SGX_BATCH_FORWARD):
        """The plan of (adj, graph_ptr, max_width, kind), kept on the adjacency's column array while both stay unchanged;
        None when the batch is not block-diagonal under graph_ptr (remembered too, so that a caller falls back without a
        device sync per call).  Where graph_ptr carries the block facts a GraphLoader recorded for this adjacency, the
        plan is the trusted one (BatchPlan.known): no device check, no synchronisation."""
        key = (BatchPlan._CACHE_KEY, adj.val.dtype, int(max_width)) + (() if kind == _lib.SGX_BATCH_FORWARD else (int(kind),))
        hit = cached_on(adj.col, key, lambda: [None, -1, None])
        if hit[0] is not graph_ptr or hit[1] != graph_ptr._version:
            facts = recorded(graph_ptr, ("block_facts",))
            if facts is not None and facts["n_rows"] == adj.n_rows and any(c() is adj.col for c in facts["cols"]):
                plan = BatchPlan.known(graph_ptr, adj.n_rows, adj.val.dtype, facts["max_graph"], max_width, kind)
            else:
                try:
                    plan = BatchPlan(adj, graph_ptr, max_width, kind)
                except _lib.SgxError as e:
                    if e.status != _lib.SGX_ERR_BLOCKS:
                        raise
                    plan = None
            hit[:] = [graph_ptr, graph_ptr._version, plan]
        return hit[2]

    _CACHE_KEY = "batch_plan"                  # cached(): entries [graph_ptr, its version, plan] on the adjacency's column array

    @staticmethod
    def cached_for(col, graph_ptr):
        """The plans cached() holds on the column array `col` for `graph_ptr` as it stands (any width, any kind)."""
        plans = []
        for key, (version, hit) in tuple(col.__dict__.get("_sgx_cache", {}).items()):
            if key[0] == BatchPlan._CACHE_KEY and version == col._version and hit[0] is graph_ptr and \
                    hit[1] == graph_ptr._version and hit[2] is not None:
                plans.append(hit[2])
        return plans

    def regroup(self, graph_ptr):
        """The trusted plan's group table written again from graph_ptr (sgx_batch_plan_regroup): the same buffer with
        the next padded batch in it -- the same n_rows, n_graphs and max_graph, other contents.  One launch, no
        synchronisation; capturable.  A plan that checked its batch on the device (BatchPlan(...)) refuses:
        SgxError SGX_ERR_UNSUPPORTED."""
        _dev(graph_ptr, "graph_ptr")
        if graph_ptr.dtype != torch.int32 or graph_ptr.numel() != self.n_graphs + 1:
            raise ValueError(f"graph_ptr must hold {self.n_graphs + 1} int32 entries, as the plan's own")
        check(lib.sgx_batch_plan_regroup(self._h, _ptr(graph_ptr), _stream()), "sgx_batch_plan_regroup")
        return self

    def export_groups(self):
        """The plan's group_graph table (first graph of every group, then n_graphs) as an int32 tensor; empty when the
        plan has none.  For tests."""
        n = lib.sgx_batch_plan_export_groups(self._h, None, 0, _stream())
        if n < 0:
            check(int(n), "sgx_batch_plan_export_groups")
        out = torch.empty(int(n), dtype=torch.int32, device="cuda")
        if n:
            got = lib.sgx_batch_plan_export_groups(self._h, _ptr(out), int(n), _stream())
            if got < 0:
                check(int(got), "sgx_batch_plan_export_groups")
        return out

    @property
    def handle(self):
        return self._h

    @property
    def rows(self):
        return lib.sgx_batch_plan_rows(self._h)

    @property
    def groups(self):
        return lib.sgx_batch_plan_groups(self._h)

    @property
    def max_graph(self):
        return lib.sgx_batch_plan_max_graph(self._h)

    @property
    def fits(self):
        return bool(lib.sgx_batch_plan_fits(self._h))

    def __del__(self, _destroy=lib.sgx_batch_plan_destroy):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _destroy(h)


# ---- shuffled graph mini-batches collated on the device (sgx_collate_graphs) -----------------------------------------
class GraphSet:
    """A graph-classification dataset uploaded once (include/sgx.h, "shuffled graph mini-batches"): the graphs collated
    in dataset order -- x (fp32), the stored edge lists in graph-local ids, y -- plus the adjacency as
    csr_from_edge_index builds it and the CSR of x, both with fp32 values, and on the host the per-graph counts every
    batch's offsets are computed from.  Building it synchronises; collating from it does not.

    graphs: pyg_lite.Graph objects (x [n, F], edge_index [2, E] in local ids 0 .. n-1, y of one element).  A graph with
    no node, an edge outside its graph, or x widths that differ: ValueError.  Graphs without edges, self loops and
    repeated edges are fine."""

    def __init__(self, graphs, device="cuda"):
        graphs = list(graphs)
        if not graphs:
            raise ValueError("GraphSet needs at least one graph")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("GraphSet lives on the GPU")
        n_nodes = np.array([g.x.shape[0] for g in graphs], dtype=np.int64)
        n_edges = np.array([g.edge_index.shape[1] for g in graphs], dtype=np.int64)
        if (n_nodes < 1).any():
            raise ValueError(f"graph {int(np.argmax(n_nodes < 1))} has no node; GraphSet refuses empty graphs")
        F = graphs[0].x.shape[1]
        if any(g.x.dim() != 2 or g.x.shape[1] != F for g in graphs):
            raise ValueError("every graph's x must be [n, F] with the same F")
        if any(g.y.numel() != 1 for g in graphs):
            raise ValueError("every graph's y must hold one label")
        ei = torch.cat([g.edge_index.reshape(2, -1).to(torch.int64).cpu() for g in graphs], dim=1)
        owner = np.repeat(np.arange(len(graphs)), n_edges)
        if ei.numel() and ((ei < 0).any() or (ei.numpy() >= n_nodes[owner][None, :]).any()):
            raise ValueError("an edge leaves its graph (edge_index must hold graph-local ids 0 .. n-1)")
        if n_nodes.sum() >= 2**31 or n_edges.sum() >= 2**31:
            raise ValueError("GraphSet holds fewer than 2^31 rows and edges")
        node_ptr = np.zeros(len(graphs) + 1, np.int64)
        np.cumsum(n_nodes, out=node_ptr[1:])
        edge_ptr = np.zeros(len(graphs) + 1, np.int64)
        np.cumsum(n_edges, out=edge_ptr[1:])
        self.device, self.n_feat, self.n_rows, self.n_edges = dev, int(F), int(node_ptr[-1]), int(edge_ptr[-1])
        self.x = torch.cat([g.x.float().cpu() for g in graphs]).to(dev).contiguous()
        self.y = torch.cat([g.y.reshape(1).to(torch.int64).cpu() for g in graphs]).to(dev)
        self.edge_index = ei.to(torch.int32).to(dev).contiguous()
        self.node_ptr = torch.as_tensor(node_ptr, dtype=torch.int32).to(dev)
        self.edge_ptr = torch.as_tensor(edge_ptr, dtype=torch.int32).to(dev)
        glob = ei + torch.as_tensor(node_ptr[owner], dtype=torch.int64).unsqueeze(0)
        self.adj = csr_from_edge_index(glob.to(dev), self.n_rows, dtype=torch.float32)
        self.fea = Csr.from_dense(self.x)
        rp_a, rp_f = self.adj.rowptr.cpu().numpy().astype(np.int64), self.fea.rowptr.cpu().numpy().astype(np.int64)
        # per-graph counts on the host: rows, stored edges, adjacency entries, feature entries
        self.counts = (n_nodes, n_edges, np.diff(rp_a[node_ptr]), np.diff(rp_f[node_ptr]))
        d = _lib.GraphSet()
        d.n_graphs, d.n_feat, d.n_edges = len(graphs), self.n_feat, self.n_edges
        d.node_ptr, d.edge_ptr = self.node_ptr.data_ptr(), self.edge_ptr.data_ptr()
        d.edge_index = self.edge_index.data_ptr() if self.n_edges else None
        d.x, d.y = self.x.data_ptr(), self.y.data_ptr()
        d.rowPtr_adj, d.columnIndex_adj, d.values_adj = self.adj.rowptr.data_ptr(), self.adj.col.data_ptr(), self.adj.val.data_ptr()
        d.rowPtr_fea, d.columnIndex_fea, d.values_fea = self.fea.rowptr.data_ptr(), self.fea.col.data_ptr(), self.fea.val.data_ptr()
        self.desc = d
        self._node_ptr_host = node_ptr
        self._sym_norm2 = None                 # the dataset-side normalised adjacency (prepare_sym_norm2), built on demand

    def __len__(self):
        return len(self.counts[0])

    def _dead_facts(self, M):
        """(dead-row mask bool [n_rows] on the device, host bool [n_graphs]: the graph has a dead row) of a dataset-side
        matrix.  One read-back."""
        dead = M.dead_rows
        run = torch.zeros(self.n_rows + 1, dtype=torch.int64, device=self.device)
        run[1:] = torch.cumsum(dead, 0)
        ptr = self.node_ptr.long()
        return dead.contiguous(), (run[ptr[1:]] > run[ptr[:-1]]).cpu().numpy()

    def prepare_sym_norm2(self, dtypes=(torch.float16,), quant=None):
        """What a batch of GAT_POOL_PYNQ needs besides the collated tensors, built ONCE for the whole set so that a batch
        only gathers it (include/sgx.h, "shuffled graph mini-batches with prepared adjacencies"): the adjacency sym_norm2
        (fill 0, unit fp32 weights) gives over the set in dataset order, as the Csr _edge_csr builds from it, its dead-row
        mask, per graph whether it has a dead row (host), per graph its entry count (host) and the set's longest row; with
        quant (a quant.QuantConstants; float32 must be among dtypes) also, for quant and quant.second_layer(), the values on
        the unsigned w_qbits grid (Csr.quantized, filed under the same key) with their mask and per-graph flags.  Cached on
        the set; every new matrix costs the torch plumbing once and one read-back.  -> GraphExtras, what
        collate_graphs(extras=) takes; dtypes: the element types the normalised values are delivered in."""
        from .sgrace import _edge_csr, sym_norm2        # (imported here: sgrace imports this module)
        dtypes = tuple(dtypes)
        for dt in dtypes:
            dtype_code(dt)
        if quant is not None and torch.float32 not in dtypes:
            raise ValueError("quant needs torch.float32 among dtypes: the quantised layer works on float32 buffers")
        p = self._sym_norm2
        if p is None:
            owner = torch.repeat_interleave(torch.arange(len(self), device=self.device),
                                            (self.edge_ptr[1:] - self.edge_ptr[:-1]).long(), output_size=self.n_edges)
            glob = self.edge_index.long() + self.node_ptr[owner].long().unsqueeze(0)
            ei, norm = sym_norm2(glob, self.n_rows)
            A = _edge_csr(None, ei, norm, self.n_rows, torch.float32)
            rp = A.rowptr.cpu().numpy().astype(np.int64)
            if rp[-1] >= 2**31:
                raise ValueError("GraphSet holds fewer than 2^31 normalised entries")
            p = self._sym_norm2 = _PreparedAdjacency(A, np.diff(rp[self._node_ptr_host]), int(np.diff(rp).max()))
            p.dead, p.has_dead = self._dead_facts(A)
        sets = _adj_quant_sets(quant)
        for key, qc in sets.items():
            if key not in p.quant:
                Q = p.adj.quantized(qc)
                p.quant[key] = (Q.val,) + self._dead_facts(Q)
        return GraphExtras(p, dtypes, tuple(sets))

    def prepare(self, idx):
        """The batch of graph ids `idx` (a host sequence, in batch order) ready to collate: its exclusive offsets
        computed here from the host counts and sent with idx through pinned memory on a non-blocking copy."""
        if isinstance(idx, torch.Tensor):
            if idx.is_cuda:
                raise ValueError("prepare takes the graph ids on the host (the offsets are computed there)")
            idx = idx.numpy()
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        B = idx.size
        if B < 1:
            raise ValueError("a batch holds at least one graph")
        if idx.min() < 0 or idx.max() >= len(self):
            raise ValueError(f"graph ids must lie in [0, {len(self)})")
        counts = self.counts if self._sym_norm2 is None else self.counts + (self._sym_norm2.counts,)
        host, totals = batch_offsets(counts, idx)
        dev = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
        return BatchIndex(dev, B, totals, int(self.counts[0][idx].max()), ids=idx)


def batch_offsets(counts, idx):
    """What GraphSet.prepare sends to the device for the graph ids idx [B]: one int32 array of idx followed by the
    exclusive offsets [B+1] of rows, stored edges, adjacency entries and feature entries (counts: those four per-graph
    count arrays; a fifth, of a prepared set: the normalised adjacency's entries), and the totals.  Host only."""
    idx = np.asarray(idx, dtype=np.int64)
    B = idx.size
    host = np.empty(B + len(counts) * (B + 1), dtype=np.int32)
    host[:B] = idx
    totals = []
    for k, c in enumerate(counts):
        off = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(np.asarray(c, dtype=np.int64)[idx], out=off[1:])
        if off[-1] >= 2**31:
            raise ValueError("a batch holds fewer than 2^31 rows, edges and entries")
        host[B + k * (B + 1): B + (k + 1) * (B + 1)] = off
        totals.append(int(off[-1]))
    return host, totals


class BatchIndex:
    """A prepared batch (GraphSet.prepare): graph ids and offsets on the device, totals and the largest graph on the
    host.  Reusable: collating the same BatchIndex again (a captured step) reads the same device buffer.  From a set
    with a prepared adjacency (GraphSet.prepare_sym_norm2) it also holds that adjacency's offsets (norm_off, nnz_norm;
    None otherwise); ids: the graph ids on the host, where the prepared batches look their per-graph facts up."""

    def __init__(self, dev, n_graphs, totals, max_graph, ids=None):
        self.dev, self.n_graphs, self.max_graph = dev, int(n_graphs), int(max_graph)
        self.n_rows, self.n_edges, self.nnz_adj, self.nnz_fea = totals[:4]
        self.ids = ids
        B = self.n_graphs
        self.index, self.node_off, self.edge_off, self.adj_off, self.fea_off = (
            dev[:B], dev[B:2 * B + 1], dev[2 * B + 1:3 * B + 2], dev[3 * B + 2:4 * B + 3], dev[4 * B + 3:5 * B + 4])
        self.norm_off, self.nnz_norm = (dev[5 * B + 4:6 * B + 5], totals[4]) if len(totals) > 4 else (None, None)

    def refill(self, src, ids=None):
        """Another batch of as many graphs copied into this one's device buffer, whose address stays -- what a recorded
        padded collation reads on its next replay.  src: the other batch's `dev` array (device int32, as batch_offsets
        lays it out), copied device to device on the current stream.  The host totals keep describing the batch this
        object was prepared for: a padded collation reads the live totals on the device."""
        if src.shape != self.dev.shape or src.dtype != self.dev.dtype:
            raise ValueError("refill takes the `dev` array of a batch of as many graphs from the same set")
        self.dev.copy_(src, non_blocking=True)
        if ids is not None:
            self.ids = ids
        return self


class PadCapacity:
    """The fixed capacity of the padded batches of one (set, batch size) (include/sgx.h, "padded batches"), host only:
    batch_size B, n_rows N, n_graphs G = B + fillers, filler_rows R_f, n_min, and the entry capacities n_edges, nnz_adj,
    nnz_fea and nnz_norm (None without a prepared adjacency)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def key(self):
        return tuple(sorted(self.__dict__.items()))

    def fits(self, n_graphs, n_rows):
        """A batch fits when it has exactly B graphs and at most N rows."""
        return n_graphs == self.batch_size and n_rows <= self.n_rows


def pad_capacity(graphset, batch_size, pad_rows=None):
    """The PadCapacity of the batches of `batch_size` graphs of `graphset` (anything with GraphSet's host `counts`; a
    prepared set's normalised adjacency counts too) by the rule of include/sgx.h: N = the sum of the B largest row
    counts, or pad_rows; n_min = the sum of the B smallest; R_f = the largest row count; F = ceil((N - n_min) / R_f)
    filler graphs; the edge and feature capacities the sums of the B largest counts, a pattern's that sum plus
    N - n_min.  Host only."""
    B = int(batch_size)
    rows = np.asarray(graphset.counts[0], dtype=np.int64)
    if not 1 <= B <= rows.size:
        raise ValueError(f"batch_size must lie in [1, {rows.size}], the graphs of the set")
    top = lambda c: int(np.sort(np.asarray(c, dtype=np.int64))[-B:].sum())
    n_min, R_f = int(np.sort(rows)[:B].sum()), int(rows.max())
    N = top(rows) if pad_rows is None else int(pad_rows)
    if N < n_min:
        raise ValueError(f"pad_rows = {N} is under the smallest batch's {n_min} rows: no batch would fit")
    spare = N - n_min
    prepared = getattr(graphset, "_sym_norm2", None)
    cap = PadCapacity(batch_size=B, n_rows=N, n_min=n_min, filler_rows=R_f, n_graphs=B + (spare + R_f - 1) // R_f,
                      n_edges=top(graphset.counts[1]), nnz_adj=top(graphset.counts[2]) + spare, nnz_fea=top(graphset.counts[3]),
                      nnz_norm=None if prepared is None else top(prepared.counts) + spare)
    if max(cap.n_rows, cap.n_edges, cap.nnz_adj, cap.nnz_fea, cap.nnz_norm or 0) >= 2**31:
        raise ValueError("a padded batch holds fewer than 2^31 rows, edges and entries")
    return cap


class _PreparedAdjacency:
    """The dataset-side state of GraphSet.prepare_sym_norm2: adj (the normalised Csr of the whole set, fp32), counts (host,
    entries per graph), max_row, dead / has_dead (device mask, host per-graph flags) and quant {key: (values, dead,
    has_dead)}."""

    def __init__(self, adj, counts, max_row):
        self.adj, self.counts, self.max_row = adj, counts, max_row
        self.dead = self.has_dead = None
        self.quant = {}


class GraphExtras:
    """What collate_graphs(extras=) gathers besides the batch (GraphSet.prepare_sym_norm2): the prepared adjacency, the
    dtypes its values are delivered in and the keys (_adj_quant_key) of the quantised value arrays delivered with it."""

    def __init__(self, prepared, dtypes, keys):
        if 1 + len(keys) > _lib.SGX_COLLATE_MAX_EXTRAS:
            raise ValueError(f"a batch gathers up to {_lib.SGX_COLLATE_MAX_EXTRAS} extras")
        self.prepared, self.dtypes, self.keys = prepared, tuple(dtypes), tuple(keys)


class Collated:
    """One collated batch (collate_graphs): x [n, F] fp32, edge_index [2, E] int64, batch [n] int64, y [B] int64,
    graph_ptr [B+1] int32, the adjacency (adj_rowptr, adj_col, adj_val {dtype: values}) and the feature CSR (fea_*).
    With extras (a GraphExtras) also the normalised adjacency -- norm_rowptr, norm_col, norm_val {dtype: values}, norm_dead
    (bool [n]) -- and per quantiser key q_val {key: fp32 values over the same pattern} and q_dead {key: bool [n]}."""

    FIELDS = ("x", "edge_index", "batch", "y", "graph_ptr", "adj_rowptr", "adj_col", "fea_rowptr", "fea_col")

    def __init__(self, index, n_feat, dtypes, device, extras=None):
        e = lambda *shape, dt=torch.int32: torch.empty(shape, dtype=dt, device=device)
        i = index
        self.index, self.n_feat = i, n_feat
        self.x, self.edge_index = e(i.n_rows, n_feat, dt=torch.float32), e(2, i.n_edges, dt=torch.int64)
        self.batch, self.y, self.graph_ptr = e(i.n_rows, dt=torch.int64), e(i.n_graphs, dt=torch.int64), e(i.n_graphs + 1)
        self.adj_rowptr, self.adj_col = e(i.n_rows + 1), e(i.nnz_adj)
        self.fea_rowptr, self.fea_col = e(i.n_rows + 1), e(i.nnz_fea)
        self.adj_val = {dt: e(i.nnz_adj, dt=dt) for dt in dtypes}
        self.fea_val = {dt: e(i.nnz_fea, dt=dt) for dt in dtypes}
        self.extras = extras
        self.pad = None                        # the PadCapacity of a padded batch (collate_graphs(pad=))
        self.norm_rowptr = self.norm_col = self.norm_dead = None
        self.norm_val, self.q_val, self.q_dead = {}, {}, {}
        if extras is not None:
            self.norm_rowptr, self.norm_col = e(i.n_rows + 1), e(i.nnz_norm)
            self.norm_dead = e(i.n_rows, dt=torch.bool)
            self.norm_val = {dt: e(i.nnz_norm, dt=dt) for dt in extras.dtypes}
            self.q_val = {key: e(i.nnz_norm, dt=torch.float32) for key in extras.keys}
            self.q_dead = {key: e(i.n_rows, dt=torch.bool) for key in extras.keys}

    @classmethod
    def for_capacity(cls, pad, n_feat, dtypes, device, extras=None):
        """The buffers of the padded batches of capacity `pad` (a PadCapacity, which names its sizes as a BatchIndex
        does): every array capacity-sized, y and graph_ptr over pad.n_graphs graphs.  `index` is set by the collation."""
        self = cls(pad, n_feat, dtypes, device, extras)
        self.index, self.pad = None, pad
        return self

    def fits(self, index, n_feat, dtypes, extras=None, pad=None):
        if (self.pad is None) != (pad is None):
            return False
        if pad is not None:
            if self.pad.key() != pad.key() or (extras is not None and (self.norm_rowptr is None or not
                                                                       set(self.norm_val) >= set(extras.dtypes) or not
                                                                       set(self.q_val) >= set(extras.keys))):
                return False
            return self.n_feat == n_feat and set(self.adj_val) >= set(dtypes) and set(self.fea_val) >= set(dtypes)
        i, j = self.index, index
        if extras is not None and (self.norm_rowptr is None or i.nnz_norm != j.nnz_norm or
                                   not set(self.norm_val) >= set(extras.dtypes) or not set(self.q_val) >= set(extras.keys)):
            return False
        return ((i.n_graphs, i.n_rows, i.n_edges, i.nnz_adj, i.nnz_fea) == (j.n_graphs, j.n_rows, j.n_edges, j.nnz_adj, j.nnz_fea)
                and self.n_feat == n_feat and set(self.adj_val) >= set(dtypes) and set(self.fea_val) >= set(dtypes))


def _graph_batch(index, out, dtypes):
    """struct sgx_graph_batch of the prepared batch `index` over the buffers of the Collated `out`."""
    b = _lib.GraphBatch()
    b.n_graphs, b.n_rows = index.n_graphs, index.n_rows
    b.n_edges, b.nnz_adj, b.nnz_fea = index.n_edges, index.nnz_adj, index.nnz_fea
    b.index, b.node_off, b.edge_off = index.index.data_ptr(), index.node_off.data_ptr(), index.edge_off.data_ptr()
    b.adj_off, b.fea_off = index.adj_off.data_ptr(), index.fea_off.data_ptr()
    b.x, b.edge_index, b.batch, b.y = out.x.data_ptr(), out.edge_index.data_ptr(), out.batch.data_ptr(), out.y.data_ptr()
    b.graph_ptr = out.graph_ptr.data_ptr()
    b.rowPtr_adj, b.columnIndex_adj = out.adj_rowptr.data_ptr(), out.adj_col.data_ptr()
    b.rowPtr_fea, b.columnIndex_fea = out.fea_rowptr.data_ptr(), out.fea_col.data_ptr()
    for dt in dtypes:
        b.values_adj[dtype_code(dt)] = out.adj_val[dt].data_ptr()
        b.values_fea[dtype_code(dt)] = out.fea_val[dt].data_ptr()
    return b


def _collate_extras(index, out, extras):
    """The sgx_collate_extra array of `extras` over the buffers of `out`: the normalised adjacency (pattern, values per
    dtype, dead rows), then one entry per quantiser key over the same pattern (fp32 values and dead rows only)."""
    p = extras.prepared
    xs = (_lib.CollateExtra * _lib.SGX_COLLATE_MAX_EXTRAS)()
    for k, key in enumerate((None,) + extras.keys):
        x = xs[k]
        val, dead = (p.adj.val, p.dead) if key is None else p.quant[key][:2]
        x.rowPtr, x.columnIndex, x.values, x.dead_row = p.adj.rowptr.data_ptr(), p.adj.col.data_ptr(), val.data_ptr(), dead.data_ptr()
        x.nnz, x.entry_off = index.nnz_norm, index.norm_off.data_ptr()
        if key is None:
            x.rowPtr_out, x.columnIndex_out = out.norm_rowptr.data_ptr(), out.norm_col.data_ptr()
            for dt in extras.dtypes:
                x.values_out[dtype_code(dt)] = out.norm_val[dt].data_ptr()
            x.dead_row_out = out.norm_dead.data_ptr()
        else:
            x.values_out[SGX_F32], x.dead_row_out = out.q_val[key].data_ptr(), out.q_dead[key].data_ptr()
    return xs, 1 + len(extras.keys)


def _regroup_cached_plans(out):
    """The table launch of every trusted plan cached for the buffers of the padded Collated `out` (BatchPlan.cached keeps
    them on the adjacencies' column arrays), run again on its graph_ptr: the plan a warm-up step built follows the batch
    the buffers hold now, inside a recorded step as well."""
    for col in (out.adj_col, out.norm_col):
        for plan in (() if col is None else BatchPlan.cached_for(col, out.graph_ptr)):
            if plan.trusted:
                plan.regroup(out.graph_ptr)


def _collate_padded(graphset, index, dtypes, out, extras, pad, pad_quant=False):
    """collate_graphs(pad=): the checks, the capacity-sized Collated and the one launch of sgx_collate_graphs_padded -- with
    pad_quant of sgx_collate_graphs_padded_quant, which also pads the quantised adjacencies of extras.keys."""
    if extras is not None and extras.keys and not pad_quant:
        raise ValueError("collate_graphs: padded batches carry the quantised adjacencies (pad with quant=) only with "
                         "pad_quant=True")
    if extras is not None and pad.nnz_norm is None:
        raise ValueError("collate_graphs: `pad` was computed before graphset.prepare_sym_norm2; compute it after")
    if not pad.fits(index.n_graphs, index.n_rows):
        raise ValueError(f"collate_graphs: a batch of {index.n_graphs} graphs and {index.n_rows} rows does not fit the capacity "
                         f"of {pad.batch_size} graphs and {pad.n_rows} rows")
    if out is None:
        out = Collated.for_capacity(pad, graphset.n_feat, dtypes, graphset.device, extras)
    elif not out.fits(index, graphset.n_feat, dtypes, extras, pad):
        raise ValueError("collate_graphs: `out` was made for another capacity or other dtypes")
    out.index = index
    b = _graph_batch(index, out, dtypes)
    c = _lib.CollatePad()
    c.n_rows, c.n_graphs, c.filler_rows = pad.n_rows, pad.n_graphs, pad.filler_rows
    c.n_edges, c.nnz_adj, c.nnz_fea = pad.n_edges, pad.nnz_adj, pad.nnz_fea
    xs, n = (None, 0) if extras is None else _collate_extras(index, out, extras)
    for k in range(n):
        c.nnz_extra[k] = pad.nnz_norm
    if pad_quant:
        q = _lib.CollatePadQuant()
        for k, (bits, a_s, a_z) in enumerate(() if extras is None else extras.keys, 1):       # (extra 0: the normalised adjacency)
            q.qbits[k], q.inv_scale_adj[k], q.zero_adj[k] = int(bits), float(1 / a_s), float(a_z)
        check(lib.sgx_collate_graphs_padded_quant(ctypes.byref(graphset.desc), ctypes.byref(b), xs, n, ctypes.byref(c),
                                                  ctypes.byref(q), _stream()), "sgx_collate_graphs_padded_quant")
    else:
        check(lib.sgx_collate_graphs_padded(ctypes.byref(graphset.desc), ctypes.byref(b), xs, n, ctypes.byref(c), _stream()),
              "sgx_collate_graphs_padded")
    _regroup_cached_plans(out)
    return out


def collate_graphs(graphset, idx, dtypes=(torch.float16,), out=None, extras=None, pad=None, pad_quant=False):
    """The batch of the graphs `idx` of `graphset` in that order, built on the device by one launch of
    sgx_collate_graphs: the same x / edge_index / batch / y as pyg_lite.collate, the same adjacency as
    csr_from_edge_index, the same feature CSR as Csr.from_dense, graph_ptr as graph_ptr_of -- with the CSR values in each
    of `dtypes`.  idx: host graph ids, or a BatchIndex from graphset.prepare.  out: a Collated of the same sizes to write
    into (a captured batch); a new one otherwise.  No synchronisation.
    extras (a GraphExtras from graphset.prepare_sym_norm2): the same launch (sgx_collate_graphs_extras) also gathers the
    batch's normalised adjacency, its dead-row mask and the quantised values with theirs into out.norm_* / out.q_*.
    pad (a PadCapacity from pad_capacity(graphset, B)): the batch padded to that capacity (include/sgx.h, "padded
    batches"; one launch of sgx_collate_graphs_padded) -- every tensor has the capacity's size whatever the batch, the
    batch's graphs in the live prefix and filler graphs behind (y, graph_ptr: pad.n_graphs entries) -- and the trusted
    batch plans cached for the buffers of `out` have their tables written again, so that a recorded step which collates
    into `out` serves every batch that fits.  Extras with quantised values are refused unless pad_quant=True: the launch
    is then sgx_collate_graphs_padded_quant, which pads out.q_val / out.q_dead as well -- a filler row's diagonal entry
    holds the grid's image of 1, the spare entries its image of 0 (which must be positive and 0: SgxError otherwise)."""
    index = idx if isinstance(idx, BatchIndex) else graphset.prepare(idx)
    dtypes = tuple(dtypes)
    for dt in dtypes:
        dtype_code(dt)
    if extras is not None and (index.norm_off is None or extras.prepared is not graphset._sym_norm2):
        raise ValueError("collate_graphs: extras need a batch prepared after graphset.prepare_sym_norm2, and extras of this set")
    if pad_quant and pad is None:
        raise ValueError("collate_graphs: pad_quant goes with pad=")
    if pad is not None:
        return _collate_padded(graphset, index, dtypes, out, extras, pad, pad_quant)
    if out is None:
        out = Collated(index, graphset.n_feat, dtypes, graphset.device, extras)
    elif not out.fits(index, graphset.n_feat, dtypes, extras):
        raise ValueError("collate_graphs: `out` was made for a batch of other sizes or dtypes")
    else:
        out.index = index
    b = _graph_batch(index, out, dtypes)
    if extras is None:
        check(lib.sgx_collate_graphs(ctypes.byref(graphset.desc), ctypes.byref(b), _stream()), "sgx_collate_graphs")
    else:
        xs, n = _collate_extras(index, out, extras)
        check(lib.sgx_collate_graphs_extras(ctypes.byref(graphset.desc), ctypes.byref(b), xs, n, _stream()),
              "sgx_collate_graphs_extras")
    return out


def gcn_stack_forward(adj, x, weights_t, relus, graph_ptr, head_weight=None, head_bias=None, want_layer_outputs=False,
                      want_pooled=False, plan=None, keep=None):
    """n GCN layers, the per-graph mean and a Linear head in one call (sgx_stack_forward) -- exactly the chain
    layer_forward x n -> readout_mean_linear, bit for bit (include/sgx.h), in one launch where the batch's graphs fit
    the plan, through the chained kernels otherwise.

    adj: Csr [N, N] whose graphs are the row segments of graph_ptr (int32 [G+1]; None = one graph of all N rows);
    x: Csr features (layer 0 sparse) or a dense [N, M] tensor; weights_t: 1 to 4 tensors W_l^T [P_l, M_l] in adj's
    dtype; relus: one flag per layer.  Returns logits [G, C] fp32 with a head ((logits, pooled) with want_pooled), the
    pooled means [G, P_last] fp32 without one, or with graph_ptr None the last layer's output [N, P_last]; with
    want_layer_outputs also the list of every layer's output D_l [N, P_l] (keep: one flag per layer, which of them to
    write; the others are None)."""
    return _stack_forward(adj, x, weights_t, relus, graph_ptr, head_weight, head_bias, want_layer_outputs, want_pooled, plan,
                          keep)


def gat_stack_forward(adj, x, weights_t, attentions, relus, graph_ptr, head_weight=None, head_bias=None, alpha=0.2,
                      want_layer_outputs=False, plan=None):
    """gcn_stack_forward with a per-layer choice of the aggregate (sgx_gat_stack_forward, include/sgx.h "GAT layers in the
    small-graph stack"): attentions[l] is layer l's attention vector [2 * P_l] (a1 then a2) in adj's dtype -- the
    single-head edge softmax of gat_aggregate on H_l, rows without a live entry giving 0 -- or None for a GCN layer.  One
    launch where the batch's graphs fit the plan (the plan of gcn_stack_forward: BatchPlan.cached), the chained kernels
    otherwise.  Arguments and results as gcn_stack_forward's; alpha is the LeakyReLU slope of the scores."""
    if len(attentions) != len(weights_t):
        raise ValueError("gat_stack_forward takes one attention vector (or None) per layer")
    return _stack_forward(adj, x, weights_t, relus, graph_ptr, head_weight, head_bias, want_layer_outputs, False, plan, None,
                          attentions=list(attentions), alpha=alpha)


def quant_stack_forward(adj, x, weights_t, attentions, relus, graph_ptr, quants, head_weight=None, head_bias=None, alpha=0.2,
                        plan=None, adj_quantised=False, want_layer_outputs=False, want_pooled=False):
    """gat_stack_forward with a per-layer quantiser (sgx_quant_stack_forward, include/sgx.h "quantised layers in the
    small-graph stack"): quants[l] is layer l's quant.QuantConstants -- the layer is then layer_forward(..., quant=
    quants[l]) with the zero dead-row rule, on float32 tensors -- or None for the plain layer.  Every operand arrives
    UNQUANTISED (the quantiser is not idempotent) except the adjacency with adj_quantised=True, which is taken as stored
    (Csr.quantized(qc)).  One launch where the batch's graphs fit the plan, layer_forward per layer otherwise.  Parity of
    the quantised layer is unpinned: the reference records no quantised output.  Arguments and results as
    gcn_stack_forward's."""
    if len(attentions) != len(weights_t) or len(quants) != len(weights_t):
        raise ValueError("quant_stack_forward takes one attention vector (or None) and one QuantConstants (or None) per layer")
    return _stack_forward(adj, x, weights_t, relus, graph_ptr, head_weight, head_bias, want_layer_outputs, want_pooled, plan,
                          None, attentions=list(attentions), alpha=alpha, quants=list(quants), adj_quantised=adj_quantised)


def _stack_desc(d, adj, x, graph_ptr, n):
    """What the six stack descriptors share (struct sgx_stack_desc ... sgx_quant_stack_grad_desc), filled into d: the
    element type, the counts, graph_ptr, the adjacency and the features, sparse (a Csr: layer 0 reads it) or dense.
    -> (sparse, k_in: the width layer 0 reads).  Every route's descriptor starts here; a new route adds only its own
    per-layer fields and outputs, then _stack_call."""
    dtype, N = adj.val.dtype, adj.n_rows
    _dev(graph_ptr, "graph_ptr")
    d.dtype, d.n_layers, d.n_rows, d.n_graphs = dtype_code(dtype), n, N, graph_ptr.numel() - 1
    d.graph_ptr = graph_ptr.data_ptr()
    d.rowPtr_adj, d.columnIndex_adj, d.values_adj = adj.rowptr.data_ptr(), adj.col.data_ptr(), adj.val.data_ptr()
    if isinstance(x, Csr):
        if x.val.dtype != dtype or x.n_rows != N:
            raise ValueError("feature CSR does not match the adjacency")
        d.rowPtr_fea, d.columnIndex_fea, d.values_fea = x.rowptr.data_ptr(), x.col.data_ptr(), x.val.data_ptr()
        return True, x.n_cols
    _dev(x, "x")
    if x.dtype != dtype or x.dim() != 2 or x.shape[0] != N:
        raise ValueError(f"dense features must be [{N}, M] {dtype}")
    d.values_fea = x.data_ptr()
    return False, x.shape[1]


def _stack_call(d, name, adj, graph_ptr, plan, widths, kind):
    """The last step of every stack route: the plan of `kind` (looked up for the widest of `widths` when the caller gave
    none), the workspace of entry point `name` and the call, under check."""
    if plan is None:
        plan = BatchPlan.cached(adj, graph_ptr, max(widths), kind)
        if plan is None:
            check(_lib.SGX_ERR_BLOCKS, "sgx_batch_plan_create" if kind == _lib.SGX_BATCH_FORWARD else "sgx_batch_plan_create_ex")
    d.plan = plan.handle
    nbytes = getattr(lib, name.replace("_forward", "") + "_workspace_bytes")(ctypes.byref(d))
    if nbytes:
        ws = _workspace(adj.val.device, nbytes)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    check(getattr(lib, name)(ctypes.byref(d), _stream()), name)


def _stack_forward(adj, x, weights_t, relus, graph_ptr, head_weight, head_bias, want_layer_outputs, want_pooled, plan, keep,
                   attentions=None, alpha=0.2, quants=None, adj_quantised=False):
    """The descriptor of sgx_stack_forward (attentions None), sgx_gat_stack_forward or sgx_quant_stack_forward (quants
    given), its workspace and the call."""
    gat = attentions is not None
    label = "quant" if quants is not None else "gat" if gat else "gcn"
    n = len(weights_t)
    if not 1 <= n <= 4 or len(relus) != n:
        raise ValueError(f"{label}_stack_forward takes 1 to 4 layers and one relu flag per layer")
    dtype = adj.val.dtype
    N, dev = adj.n_rows, adj.val.device
    if adj.n_cols != N:
        raise ValueError("the adjacency must be square")
    readout = graph_ptr is not None
    if graph_ptr is None:
        graph_ptr = cached_on(adj.rowptr, ("one_graph_ptr",),
                              lambda: torch.tensor([0, N], dtype=torch.int32, device=dev))
    d = _lib.QuantStackDesc() if quants is not None else _lib.GatStackDesc() if gat else _lib.StackDesc()
    sparse, k_in = _stack_desc(d, adj, x, graph_ptr, n)
    qstructs = []                                                                              # (held until the call returns)
    outs = []
    widths = []
    for l, (Wt, relu) in enumerate(zip(weights_t, relus)):
        _dev(Wt, f"weights_t[{l}]")
        P, M = Wt.shape
        if Wt.dtype != dtype or M != k_in:
            raise ValueError(f"weights_t[{l}] must be [P, {k_in}] {dtype}, got {tuple(Wt.shape)} {Wt.dtype}")
        L = d.layer[l]
        L.gemm_mode = 0 if (l == 0 and sparse) else 1
        L.relu, L.M_fea, L.P_w, L.B = int(bool(relu)), M, P, Wt.data_ptr()
        if gat and attentions[l] is not None:
            att = attentions[l] = _dev(attentions[l], f"attentions[{l}]").reshape(-1)      # (held until the call returns)
            if att.dtype != dtype or att.numel() != 2 * P:
                raise ValueError(f"attentions[{l}] must hold 2 * {P} elements of {dtype}")
            L.gat_mode, L.attention, L.alpha = 1, att.data_ptr(), float(alpha)
        if quants is not None and quants[l] is not None:
            qstructs.append(quants[l].as_struct(nnz_adj=adj.nnz, nnz_fea=x.nnz if (l == 0 and sparse) else 0,
                                                adj_done=adj_quantised))
            L.quant = ctypes.pointer(qstructs[-1])
        if (want_layer_outputs and (keep is None or keep[l])) or (not readout and l == n - 1):
            D = torch.empty((N, P), dtype=dtype, device=dev)
            L.D, L.ldd = D.data_ptr(), P
            outs.append(D)
        elif want_layer_outputs:
            outs.append(None)
        widths += [P] if (l == 0 and sparse) else [P, M]
        k_in = P
    G = d.n_graphs
    pooled = logits = None
    if readout:
        if head_weight is not None:
            w = _dev(head_weight.detach().float().contiguous(), "head_weight")
            if w.dim() != 2 or w.shape[1] != k_in:
                raise ValueError(f"head_weight must be [C, {k_in}]")
            d.C, d.W_head = w.shape[0], w.data_ptr()
            if head_bias is not None:
                b = _dev(head_bias.detach().float().contiguous(), "head_bias")
                d.bias = b.data_ptr()
            logits = torch.empty((G, d.C), dtype=torch.float32, device=dev)
            d.logits = logits.data_ptr()
        if head_weight is None or want_pooled:
            pooled = torch.empty((G, k_in), dtype=torch.float32, device=dev)
            d.pooled = pooled.data_ptr()
    _stack_call(d, f"sgx_{'' if label == 'gcn' else label + '_'}stack_forward", adj, graph_ptr, plan, widths,
                _lib.SGX_BATCH_FORWARD)
    if not readout:
        out = outs[-1]
    elif logits is not None:
        out = (logits, pooled) if want_pooled else logits
    else:
        out = pooled
    return (out, outs) if want_layer_outputs else out


# ---- the backward of that stack for training (sgx_stack_backward, sgx_gat_stack_backward, sgx_quant_stack_backward) ----
def gcn_stack_backward(adj, x, weights, relus, graph_ptr, layer_outputs, grad_pooled, plan=None, want_G=False):
    """Weight gradients of the stack sgx_stack_forward ran (include/sgx.h, "training"): one launch over the batch's graphs
    and one reduction.  weights: the fp32 parameters W_l [M_l, P_l] (not transposed); layer_outputs: the forward's D_l
    in adj's dtype (D_{L-1} may be None unless the last layer has ReLU); grad_pooled [G, P_last] fp32.  Returns the
    list of dW_l [M_l, P_l] fp32 (and the list of G_l = A . g_l [N, P_l] fp32 with want_G).  plan: an SGX_BATCH_BACKWARD
    BatchPlan (built and cached when None).  Raises SgxError SGX_ERR_UNSUPPORTED where the batch or the widths are
    outside the kernel's limits -- the caller then runs the layers one by one."""
    grads, _, Gs, _ = _stack_backward(adj, x, weights, None, relus, graph_ptr, layer_outputs, grad_pooled, 0.2, plan, want_G,
                                      False)
    return (grads, Gs) if want_G else grads


def gat_stack_backward(adj, x, weights, attentions, relus, graph_ptr, layer_outputs, grad_pooled, alpha=0.2, plan=None,
                       want_G=False, want_edge_outputs=False):
    """gcn_stack_backward with a per-layer choice of P in G_l = P . g_l (include/sgx.h, "training the GAT stack"):
    attentions[l] is layer l's fp32 attention parameter (2 * P_l elements, a1 then a2) -- P is then the layer's edge
    softmax, formed again from X_l and the fp32 parameters -- or None for a GCN layer (P = the adjacency).  The other
    arguments are gcn_stack_backward's.  Returns (dW list, grad_attention list -- [2 * P_l] fp32, None for a GCN layer
    [, G list] [, (E, S) list -- [nnz] fp32 each, None for a GCN layer]).  Raises SgxError SGX_ERR_UNSUPPORTED where the
    batch or the widths are outside the kernel's limits -- the caller then runs the layers one by one."""
    grads, gatts, Gs, edges = _stack_backward(adj, x, weights, list(attentions), relus, graph_ptr, layer_outputs, grad_pooled,
                                              alpha, plan, want_G, want_edge_outputs)
    return (grads, gatts) + ((Gs,) if want_G else ()) + ((edges,) if want_edge_outputs else ())


def quant_stack_backward(adj, x, weights, attentions, relus, graph_ptr, layer_outputs, grad_pooled, quants, alpha=0.2, plan=None,
                         adj_q=None, want_G=False, want_edge_outputs=False):
    """gat_stack_backward with a per-layer quantiser (include/sgx.h, "training the quantised stack"): the backward of the
    stack quant_stack_forward ran, by FPYNQ_GAT.backward's rule under fake quantisation.  quants[l] is layer l's
    quant.QuantConstants or None.  A quantised GAT layer's attention matrix is the quantised forward's S, formed again in
    the kernel (X_l, W_l and the attention vector on their grids, H requantised, the mask on the quantised adjacency);
    everything a gradient multiplies with -- X_l, W_l, Wh, a GCN layer's adjacency -- is unquantised, and deq_factor
    reaches no gradient.  adj: the UNQUANTISED float32 adjacency; adj_q: adj.quantized(qc), taken as stored for the masks
    (None: adj's values are quantised as they are read); layer_outputs: the quantised forward's D_l.  Returns what
    gat_stack_backward returns.  Parity of the quantised layer is unpinned."""
    grads, gatts, Gs, edges = _stack_backward(adj, x, weights, list(attentions), relus, graph_ptr, layer_outputs, grad_pooled,
                                              alpha, plan, want_G, want_edge_outputs, quants=list(quants), adj_q=adj_q)
    return (grads, gatts) + ((Gs,) if want_G else ()) + ((edges,) if want_edge_outputs else ())


def _stack_backward(adj, x, weights, attentions, relus, graph_ptr, layer_outputs, grad_pooled, alpha, plan, want_G,
                    want_edge_outputs, quants=None, adj_q=None):
    """The descriptor of sgx_stack_backward (attentions None: an sgx_stack_grad_desc, no attention field is touched),
    sgx_gat_stack_backward or sgx_quant_stack_backward (quants given), its workspace and the call.
    -> (dW list, grad_attention list, G list, (E, S) list), the last three as far as they were asked for."""
    label = "quant" if quants is not None else "gat" if attentions is not None else "gcn"
    n = len(weights)
    per_layer = [relus, layer_outputs] + [v for v in (attentions, quants) if v is not None]
    if not 1 <= n <= 4 or any(len(v) != n for v in per_layer):
        raise ValueError(f"{label}_stack_backward takes 1 to 4 layers; "
                         + ("one attention vector (or None), " if attentions is not None else "")
                         + "one relu flag and one layer output per layer"
                         + (", one QuantConstants (or None) per layer" if quants is not None else ""))
    dtype = adj.val.dtype
    N, dev = adj.n_rows, adj.val.device
    d = {"gcn": _lib.StackGradDesc, "gat": _lib.GatStackGradDesc, "quant": _lib.QuantStackGradDesc}[label]()
    if adj_q is not None:
        if quants is None:
            raise ValueError("adj_q goes with quants: gat_stack_backward has no quantised adjacency")
        if adj_q.val.dtype != torch.float32 or adj_q.nnz != adj.nnz or adj_q.n_rows != N:
            raise ValueError("adj_q must be the float32 quantised values on adj's pattern")
        d.values_adj_q = adj_q.val.data_ptr()
    sparse, k_in = _stack_desc(d, adj, x, graph_ptr, n)
    grads, gatts, Gs, edges, widths = [], [], [], [], []
    held = []                                                            # (fp32 copies and structs, held until the call returns)
    for l, (W, att, relu, D) in enumerate(zip(weights, attentions or [None] * n, relus, layer_outputs)):
        W = _dev(W.detach().float().contiguous(), f"weights[{l}]")
        M, P = W.shape
        if M != k_in:
            raise ValueError(f"weights[{l}] must be [{k_in}, P], got {tuple(W.shape)}")
        L = d.layer[l]
        L.gemm_mode = 0 if (l == 0 and sparse) else 1
        L.relu, L.M_fea, L.P_w, L.W = int(bool(relu)), M, P, W.data_ptr()
        if D is not None:
            _dev2d(D, f"layer_outputs[{l}]")
            if D.dtype != dtype or D.shape != (N, P):
                raise ValueError(f"layer_outputs[{l}] must be [{N}, {P}] {dtype}")
            L.D, L.ldd = D.data_ptr(), D.stride(0)
        gW = torch.empty((M, P), dtype=torch.float32, device=dev)
        L.grad_W = gW.data_ptr()
        grads.append(gW)
        ga = ES = None
        if att is not None:
            att = _dev(att.detach().float().reshape(-1).contiguous(), f"attentions[{l}]")
            if att.numel() != 2 * P:
                raise ValueError(f"attentions[{l}] must hold 2 * {P} elements")
            ga = torch.empty(2 * P, dtype=torch.float32, device=dev)
            L.gat_mode, L.attention, L.alpha, L.grad_attention = 1, att.data_ptr(), float(alpha), ga.data_ptr()
            if want_edge_outputs:
                ES = (torch.zeros(adj.nnz, dtype=torch.float32, device=dev), torch.zeros(adj.nnz, dtype=torch.float32, device=dev))
                L.E, L.S = ES[0].data_ptr(), ES[1].data_ptr()
        if quants is not None and quants[l] is not None:
            held.append(quants[l].as_struct(nnz_adj=adj.nnz, nnz_fea=x.nnz if (l == 0 and sparse) else 0,
                                            adj_done=adj_q is not None))
            L.quant = ctypes.pointer(held[-1])
        gatts.append(ga)
        edges.append(ES)
        if want_G:
            G = torch.empty((N, P), dtype=torch.float32, device=dev)
            L.G = G.data_ptr()
            Gs.append(G)
        held.append((W, att))
        widths += [P] if (l == 0 and sparse) else [P, M]
        k_in = P
    g = _dev(grad_pooled.detach().float().contiguous(), "grad_pooled")
    if g.shape != (d.n_graphs, k_in):
        raise ValueError(f"grad_pooled must be [{d.n_graphs}, {k_in}]")
    d.grad_pooled = g.data_ptr()
    _stack_call(d, f"sgx_{'' if label == 'gcn' else label + '_'}stack_backward", adj, graph_ptr, plan, widths,
                _lib.SGX_BATCH_BACKWARD)
    return grads, gatts, Gs, edges


# ---- the three stacks as autograd functions ------------------------------------------------------------------------------
def _stack_fn_forward(ctx, name, n_leading, adj, adj_q, x, graph_ptr, plan, relus, alpha, quants, params):
    """forward of GcnStack (alpha None: params are the weights), GatStack (quants None) and QuantStack: the stack's forward
    call without a head, and on ctx what _stack_fn_backward needs.  n_leading: how many arguments precede the parameters."""
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise ValueError(f"{name} gives no gradient for the features; x must not require grad")
    n = len(relus)
    gcn = alpha is None
    if not gcn and (len(params) != 2 * n or (quants is not None and len(quants) != n)):
        raise ValueError(f"{name} takes one weight" + (" and" if quants is None else ",") + " one attention vector (or None)"
                         + ("" if quants is None else " and one quantiser (or None)") + " per layer")
    weights, atts = (params, ()) if gcn else (params[:n], params[n:])
    dtype = adj.val.dtype
    wts = [torch.transpose(w, 0, 1).detach().to(dtype).contiguous() for w in weights]
    ats = [None if a is None else a.detach().to(dtype).reshape(-1).contiguous() for a in atts]
    if gcn:
        # the last layer's D is read by the backward only through that layer's ReLU mask
        keep = [l < len(wts) - 1 or bool(relus[l]) for l in range(len(wts))]
        pooled, outs = gcn_stack_forward(adj, x, wts, relus, graph_ptr, want_layer_outputs=True, plan=plan, keep=keep)
    elif quants is None:
        pooled, outs = gat_stack_forward(adj, x, wts, ats, relus, graph_ptr, alpha=alpha, want_layer_outputs=True, plan=plan)
    else:
        pooled, outs = quant_stack_forward(adj if adj_q is None else adj_q, x, wts, ats, relus, graph_ptr, list(quants),
                                           alpha=alpha, plan=plan, adj_quantised=adj_q is not None, want_layer_outputs=True)
    ctx.stack = (n_leading, adj, adj_q, x, plan, list(relus), alpha, None if quants is None else list(quants))
    ctx.kept, ctx.gat = [D is not None for D in outs], [a is not None for a in atts]
    ctx.save_for_backward(graph_ptr, *[D for D in outs if D is not None], *weights, *[a for a in atts if a is not None])
    return pooled


def _stack_fn_backward(ctx, grad_pooled):
    """backward of the three: the stack's backward call on what forward saved -> one None per leading argument, then the
    fp32 gradients of the weights and of the attention vectors in their parameters' shapes."""
    n_leading, adj, adj_q, x, plan, relus, alpha, quants = ctx.stack
    graph_ptr, *rest = ctx.saved_tensors
    outs = [rest.pop(0) if k else None for k in ctx.kept]
    weights = [rest.pop(0) for _ in ctx.kept]
    atts = [rest.pop(0) if g else None for g in ctx.gat]
    if alpha is None:
        dW, dA = gcn_stack_backward(adj, x, weights, relus, graph_ptr, outs, grad_pooled, plan=plan), ()
    elif quants is None:
        dW, dA = gat_stack_backward(adj, x, weights, atts, relus, graph_ptr, outs, grad_pooled, alpha=alpha, plan=plan)
    else:
        dW, dA = quant_stack_backward(adj, x, weights, atts, relus, graph_ptr, outs, grad_pooled, quants, alpha=alpha, plan=plan,
                                      adj_q=adj_q)
    dA = [None if g is None else g.reshape(a.shape) for g, a in zip(dA, atts)]
    return (None,) * n_leading + tuple(dW) + tuple(dA)


class GcnStack(torch.autograd.Function):
    """The GCN stack of a training step as two calls: forward = sgx_stack_forward without a head (the pooled fp32 means
    [G, P_last], the D_l the backward reads saved), backward = sgx_stack_backward (fp32 gradients of the weight
    parameters, [in, out] as FPYNQ.backward returns them).  No gradient for the features: a feature tensor that needs
    one is refused.

        pooled = GcnStack.apply(adj, x, graph_ptr, plan, relus, W_0, ..., W_{L-1})

    adj: Csr in the accelerator's dtype; x: Csr or dense features in that dtype; plan: an SGX_BATCH_BACKWARD BatchPlan
    that fits; W_l: the fp32 parameters [M_l, P_l]."""

    @staticmethod
    def forward(ctx, adj, x, graph_ptr, plan, relus, *weights):
        return _stack_fn_forward(ctx, "GcnStack", 5, adj, None, x, graph_ptr, plan, relus, None, None, weights)

    backward = staticmethod(_stack_fn_backward)


class GatStack(torch.autograd.Function):
    """GcnStack with GAT layers: forward = sgx_gat_stack_forward without a head (the pooled fp32 means, every D_l saved),
    backward = sgx_gat_stack_backward (fp32 gradients of the weights [in, out] and of the attention vectors [2 P, 1], as
    FPYNQ_GAT.backward returns them).  No gradient for the features: a feature tensor that needs one is refused.

        pooled = GatStack.apply(adj, x, graph_ptr, plan, relus, alpha, W_0, ..., W_{L-1}, a_0, ..., a_{L-1})

    plan: an SGX_BATCH_BACKWARD BatchPlan that fits; W_l: the fp32 parameters [M_l, P_l]; a_l: the fp32 attention
    parameter [2 P_l, 1], or None for a GCN layer."""

    @staticmethod
    def forward(ctx, adj, x, graph_ptr, plan, relus, alpha, *params):
        return _stack_fn_forward(ctx, "GatStack", 6, adj, None, x, graph_ptr, plan, relus, alpha, None, params)

    backward = staticmethod(_stack_fn_backward)


class QuantStack(torch.autograd.Function):
    """GatStack with a per-layer quantiser: forward = sgx_quant_stack_forward without a head (the pooled fp32 means, every
    D_l saved), backward = sgx_quant_stack_backward.  No gradient for the features.

        pooled = QuantStack.apply(adj, adj_q, x, graph_ptr, plan, relus, alpha, quants, W_0, ..., W_{L-1}, a_0, ..., a_{L-1})

    adj: the unquantised float32 Csr; adj_q: adj.quantized(qc) (the forward aggregates and both passes mask with it as
    stored) or None (adj is quantised as it is read); quants: one quant.QuantConstants (or None) per layer; the other
    arguments are GatStack's."""

    @staticmethod
    def forward(ctx, adj, adj_q, x, graph_ptr, plan, relus, alpha, quants, *params):
        return _stack_fn_forward(ctx, "QuantStack", 8, adj, adj_q, x, graph_ptr, plan, relus, alpha, quants, params)

    backward = staticmethod(_stack_fn_backward)


# ---- the tail of a training step: the loss head and the optimiser (sgx_head_loss, sgx_adam_step) ----------------------------
def _loss_operands(fn, rows_name, rows, weight, bias, target, step_dev):
    """The operand check head_loss and node_loss share -> (rows, weight, bias) detached: float32 tensors on the device,
    int64 targets, rows [n, P] against weight [C, P], bias [C] and target [n]; step_dev a device int64 tensor or None."""
    rows = _dev(rows.detach(), rows_name)
    w = _dev(weight.detach(), "weight")
    b = None if bias is None else _dev(bias.detach(), "bias")
    _dev(target, "target")
    if rows.dtype != torch.float32 or w.dtype != torch.float32 or (b is not None and b.dtype != torch.float32):
        raise TypeError(f"{fn} works on float32 tensors")
    if target.dtype != torch.int64:
        raise TypeError(f"{fn} takes int64 targets")
    if rows.dim() != 2 or w.dim() != 2 or w.shape[1] != rows.shape[1] or target.shape != (rows.shape[0],) or \
            (b is not None and b.shape != (w.shape[0],)):
        n = "G" if fn == "head_loss" else "n"
        raise ValueError(f"{fn} takes {rows_name} [{n}, P], weight [C, P], bias [C], target [{n}]")
    if step_dev is not None:
        _dev(step_dev, "step_dev")
        if step_dev.dtype != torch.int64 or step_dev.numel() < 1:
            raise TypeError("step_dev must be a device int64 tensor")
    return rows, w, b


def _loss_outputs(rows, w, b, grads, want_logits):
    """(loss [1], grad_rows, grad_W, grad_bias, logits) of a loss head over `rows`: fp32 buffers for the call to fill, None
    for what was not asked for."""
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=rows.device)
    C = w.shape[0]
    return (f32(1), f32(*rows.shape) if grads else None, f32(*w.shape) if grads else None,
            f32(C) if grads and b is not None else None, f32(rows.shape[0], C) if want_logits else None)


def _u64(v):
    return int(v) & (2 ** 64 - 1)


def _tail_workspace(device, nbytes):
    """(pointer, bytes) of a tail entry's workspace of `nbytes`, (None, 0) where it asks for none."""
    ws = _workspace(device, nbytes) if nbytes else None
    return _ptr(ws), 0 if ws is None else ws.numel()


def _row_selection(mask, n_prefix, n):
    """node_loss's and node_eval's selection, normalised -> (mask as uint8 bytes or None, n_prefix as an int, default n)."""
    if mask is not None:
        _dev(mask, "mask")
        if mask.dtype not in (torch.bool, torch.uint8) or mask.shape != (n,):
            raise TypeError("mask must be a bool or uint8 tensor [n]")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    return mask, n if n_prefix is None else int(n_prefix)


def _eval_accumulators(fn, totals, loss_sum):
    """The check of the device accumulators head_eval and node_eval add into."""
    _dev(totals, "totals"), _dev(loss_sum, "loss_sum")
    if totals.dtype != torch.int64 or totals.numel() != 2 or loss_sum.dtype != torch.float64 or loss_sum.numel() != 1:
        raise TypeError(f"{fn} accumulates into totals int64 [2] and loss_sum float64 [1]")


def head_loss(pooled, weight, bias, target, p=0.0, seed=0, step=0, step_dev=None, grad_scale=1.0, want_logits=False):
    """Dropout(p), the Linear head and the mean cross entropy with every gradient, in one call (sgx_head_loss; the rule is
    in include/sgx.h, "the loss head").  pooled [G, P] fp32, weight [C, P] fp32, bias [C] fp32 or None, target [G] int64;
    the dropout mask is a fixed function of (seed, step + step_dev[0], element); step_dev: a device int64 tensor (the
    optimiser's counter) or None.  Returns (loss [1], grad_pooled [G, P], grad_W [C, P], grad_bias [C] or None), and the
    logits [G, C] behind them with want_logits.  Never synchronises."""
    pooled, w, b = _loss_operands("head_loss", "pooled", pooled, weight, bias, target, step_dev)
    (G, P), C = pooled.shape, w.shape[0]
    loss, grad_pooled, grad_W, grad_b, logits = _loss_outputs(pooled, w, b, True, want_logits)
    ws = _tail_workspace(pooled.device, lib.sgx_head_loss_workspace_bytes(G, P, C))
    check(lib.sgx_head_loss(G, P, C, _ptr(pooled), _ptr(w), _ptr(b), _ptr(target), float(p), _u64(seed), _u64(step),
                            _ptr(step_dev), float(grad_scale), _ptr(loss), _ptr(logits), _ptr(grad_pooled), _ptr(grad_W),
                            _ptr(grad_b), *ws, _stream()),
          "sgx_head_loss")
    out = (loss, grad_pooled, grad_W, grad_b)
    return out + (logits,) if want_logits else out


class _LossFn(torch.autograd.Function):
    """What HeadLoss and NodeLoss share: forward (_run) makes the one call with grad_scale 1 and keeps its gradients,
    backward hands them on times grad_output; no other argument has a gradient."""

    @staticmethod
    def _run(ctx, call, *args):
        loss, gx, gw, gb = call(*args)
        ctx.save_for_backward(gx, gw, *([] if gb is None else [gb]))
        ctx.n_rest = len(args) - 3
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        gx, gw, *gb = ctx.saved_tensors
        return (gx * grad_output, gw * grad_output, gb[0] * grad_output if gb else None) + (None,) * ctx.n_rest


class HeadLoss(_LossFn):
    """head_loss inside an ordinary autograd loop: forward runs the one call (with grad_scale 1) and keeps its gradients,
    backward hands them on times grad_output.

        loss = HeadLoss.apply(pooled, weight, bias, target, p, seed, step, step_dev)        # a 0-dim tensor"""

    @staticmethod
    def forward(ctx, pooled, weight, bias, target, p=0.0, seed=0, step=0, step_dev=None):
        return _LossFn._run(ctx, head_loss, pooled, weight, bias, target, p, seed, step, step_dev)


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              transposed_out=None):
    """torch.optim.Adam's update (no amsgrad) of up to 16 tensors in one launch (sgx_adam_step; the rule is in
    include/sgx.h, "the optimiser").  params, exp_avgs, exp_avg_sqs: fp32 tensors updated in place; grads: fp32 tensors,
    None = that parameter is skipped; step: the device int64 counter [1], t - 1 before and t after the call.
    transposed_out: per parameter None or a [cols, rows] fp16 / fp32 tensor that receives the updated 2-D parameter
    transposed and cast.  More than 16 tensors: ValueError (one call is one step of the counter).  Never synchronises."""
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == n):
        raise ValueError("adam_step takes one gradient (or None), one exp_avg and one exp_avg_sq per parameter")
    _dev(step, "step")
    if step.dtype != torch.int64 or step.numel() != 1:
        raise TypeError("step must be a device int64 tensor of one element")
    entries = []
    for k in range(n):
        p, g = params[k].detach(), grads[k]
        if g is None or p.numel() == 0:           # the call skips these itself, as torch skips p.grad is None
            entries.append((p, None, None, None, None))
            continue
        for name, t in (("param", p), ("grad", g), ("exp_avg", exp_avgs[k]), ("exp_avg_sq", exp_avg_sqs[k])):
            _dev(t, name)
            if t.dtype != torch.float32 or t.numel() != p.numel():
                raise ValueError(f"{name}[{k}] must be a float32 tensor of the parameter's size")
        t_out = None if transposed_out is None else transposed_out[k]
        if t_out is not None:
            _dev(t_out, "transposed_out")
            if p.dim() != 2 or t_out.shape != (p.shape[1], p.shape[0]):
                raise ValueError(f"transposed_out[{k}] must be [{p.shape[-1]}, {p.shape[0]}]")
        entries.append((p, g, exp_avgs[k], exp_avg_sqs[k], t_out))
    if len(entries) > _lib.SGX_ADAM_MAX_TENSORS:
        raise ValueError(f"adam_step takes at most {_lib.SGX_ADAM_MAX_TENSORS} tensors in a call (got {len(entries)})")
    d = _lib.AdamDesc()
    d.n_tensors = len(entries)
    d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    d.step = step.data_ptr()
    for k, (p, g, m, v, t_out) in enumerate(entries):
        T = d.tensor[k]
        T.n = p.numel()
        if g is None:
            continue
        T.param, T.m, T.v, T.grad = p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr()
        if t_out is not None:
            T.param_t_out, T.dtype_t, T.rows, T.cols = t_out.data_ptr(), dtype_code(t_out.dtype), p.shape[0], p.shape[1]
    check(lib.sgx_adam_step(ctypes.byref(d), _stream()), "sgx_adam_step")


# ---- model selection: the best epoch's weights kept on the device (sgx_keep_best) --------------------------------------------
def keep_best(params, snapshot, sums, state, log=None):
    """One epoch of model selection in one call (sgx_keep_best; the rule is in include/sgx.h, "model selection"): where
    the counts in sums[0] beat the best so far -- hits * best_n > best_hits * n, in integers -- every params[k] is copied
    into snapshot[k] bit for bit and `state` takes the epoch; in every call the sums go to row `epoch` of `log` and the
    epoch advances.  params, snapshot: up to 16 fp32 tensors of equal sizes, pair by pair distinct; sums: 1 to 4 device
    int64 [3] buffers (train.EvalSums.buffer: rows, hits, the loss sum's bits), the first decides; state: a device int64
    [4] = (best_n, best_hits, best_epoch, epoch), fresh as (1, 0, -1, 0); log: None or a device int64 [rows, 3 * len(sums)].
    More than 16 tensors: ValueError.  Never synchronises."""
    n = len(params)
    if len(snapshot) != n:
        raise ValueError("keep_best takes one snapshot tensor per parameter")
    if n > _lib.SGX_BEST_MAX_TENSORS:
        raise ValueError(f"keep_best takes at most {_lib.SGX_BEST_MAX_TENSORS} tensors in a call (got {n})")
    if not 1 <= len(sums) <= _lib.SGX_BEST_MAX_SUMS:
        raise ValueError(f"keep_best takes 1 to {_lib.SGX_BEST_MAX_SUMS} sums (got {len(sums)})")
    _dev(state, "state")
    if state.dtype != torch.int64 or state.numel() != 4:
        raise TypeError("state must be a device int64 tensor of four elements")
    for k, s in enumerate(sums):
        _dev(s, f"sums[{k}]")
        if s.dtype != torch.int64 or s.numel() != 3 or s.device != state.device:
            raise TypeError(f"sums[{k}] must be an int64 tensor of three elements on the state's device")
    if log is not None:
        _dev(log, "log")
        if log.dtype != torch.int64 or log.dim() != 2 or log.shape[1] != 3 * len(sums) or log.device != state.device:
            raise TypeError(f"log must be an int64 tensor [rows, {3 * len(sums)}] on the state's device")
    d = _lib.BestDesc()
    d.n_tensors, d.n_sums = n, len(sums)
    for k in range(n):
        p, s = params[k].detach(), snapshot[k].detach()
        for name, t in (("params", p), ("snapshot", s)):
            _dev(t, f"{name}[{k}]")
            if t.dtype != torch.float32 or t.device != state.device:
                raise ValueError(f"{name}[{k}] must be a float32 tensor on the state's device")
        if s.numel() != p.numel():
            raise ValueError(f"snapshot[{k}] must have the size of params[{k}]")
        T = d.tensor[k]
        T.n = p.numel()
        if T.n:
            if p.data_ptr() == s.data_ptr():
                raise ValueError(f"snapshot[{k}] is params[{k}] itself")
            T.src, T.dst = p.data_ptr(), s.data_ptr()
    for k, s in enumerate(sums):
        d.sums[k] = s.data_ptr()
    d.state = state.data_ptr()
    if log is not None and log.shape[0] > 0:
        d.log, d.log_rows = log.data_ptr(), log.shape[0]
    check(lib.sgx_keep_best(ctypes.byref(d), _stream()), "sgx_keep_best")


# ---- the tail of a node-classification step: the loss head over selected rows (sgx_node_loss) ----------------------------------
def node_loss(H, weight, bias, target, mask=None, n_prefix=None, p=0.0, seed=0, step=0, step_dev=None, grad_scale=1.0,
              want_logits=False, want_counts=False, grads=True):
    """Dropout(p), the Linear head and the mean cross entropy over the SELECTED rows of H with every gradient, in one call
    (sgx_node_loss; the rule is in include/sgx.h, "the node loss head").  H [n, P] fp32, weight [C, P] fp32, bias [C] fp32
    or None, target [n] int64; row i is selected iff i < n_prefix (default n) and mask[i] (a bool or uint8 tensor [n],
    passed as its bytes; None: every row).  The count of selected rows stays on the device.  Returns
    (loss [1], grad_H [n, P], grad_W [C, P], grad_bias [C] or None) -- the three gradients None with grads=False, the
    evaluation mode -- then counts (int64 [2]: selected rows, arg-max hits among them) with want_counts and the logits
    [n, C] of every row with want_logits.  Never synchronises."""
    H, w, b = _loss_operands("node_loss", "H", H, weight, bias, target, step_dev)
    (n, P), C = H.shape, w.shape[0]
    mask, n_prefix = _row_selection(mask, n_prefix, n)
    loss, grad_H, grad_W, grad_b, logits = _loss_outputs(H, w, b, grads, want_logits)
    counts = torch.empty(2, dtype=torch.int64, device=H.device) if want_counts else None
    ws = _tail_workspace(H.device, lib.sgx_node_loss_workspace_bytes(n, P, C))
    check(lib.sgx_node_loss(n, n_prefix, P, C, _ptr(H), _ptr(w), _ptr(b), _ptr(target), _ptr(mask), float(p), _u64(seed),
                            _u64(step), _ptr(step_dev), float(grad_scale), _ptr(loss), _ptr(counts), _ptr(logits), _ptr(grad_H),
                            _ptr(grad_W), _ptr(grad_b), *ws, _stream()),
          "sgx_node_loss")
    out = (loss, grad_H, grad_W, grad_b)
    if want_counts:
        out = out + (counts,)
    return out + (logits,) if want_logits else out


class NodeLoss(_LossFn):
    """node_loss inside an ordinary autograd loop: forward runs the one call (with grad_scale 1) and keeps its gradients,
    backward hands them on times grad_output.

        loss = NodeLoss.apply(H, weight, bias, target, mask, n_prefix, p, seed, step, step_dev)        # a 0-dim tensor"""

    @staticmethod
    def forward(ctx, H, weight, bias, target, mask=None, n_prefix=None, p=0.0, seed=0, step=0, step_dev=None):
        return _LossFn._run(ctx, node_loss, H, weight, bias, target, mask, n_prefix, p, seed, step, step_dev)


# ---- the tail of an evaluation pass: hits and the summed loss, kept on the device across batches (sgx_head_eval) ---------------
def head_eval(pooled, weight, bias, target, n_real=None, totals=None, loss_sum=None, want_logits=False):
    """The Linear head, the arg-max's hits and the summed cross entropy of the first n_real rows (default: all) of pooled,
    ADDED to accumulators that stay on the device, in one launch (sgx_head_eval; the rule is in include/sgx.h, "the
    evaluation head").  pooled [G, P] fp32, weight [C, P] fp32, bias [C] fp32 or None, target [G] int64; rows n_real ..
    G - 1, the filler graphs of a padded batch, reach no sum.  totals: a device int64 [2] that receives += (n_real, hits);
    loss_sum: a device float64 [1] that receives += the rows' losses; zeroed ones are made where none is passed.  Returns
    (totals, loss_sum), and the logits [G, C] of every row behind them with want_logits.  Never synchronises."""
    pooled, w, b = _loss_operands("head_eval", "pooled", pooled, weight, bias, target, None)
    (G, P), C = pooled.shape, w.shape[0]
    n_real = G if n_real is None else int(n_real)
    if not 0 <= n_real <= G:
        raise ValueError(f"head_eval: n_real = {n_real} is outside 0 .. G = {G}")
    if totals is None:
        totals = torch.zeros(2, dtype=torch.int64, device=pooled.device)
    if loss_sum is None:
        loss_sum = torch.zeros(1, dtype=torch.float64, device=pooled.device)
    _eval_accumulators("head_eval", totals, loss_sum)
    logits = torch.empty((G, C), dtype=torch.float32, device=pooled.device) if want_logits else None
    ws = _tail_workspace(pooled.device, lib.sgx_head_eval_workspace_bytes(G, P, C))
    check(lib.sgx_head_eval(G, n_real, P, C, _ptr(pooled), _ptr(w), _ptr(b), _ptr(target), _ptr(totals), _ptr(loss_sum),
                            _ptr(logits), *ws, _stream()),
          "sgx_head_eval")
    return (totals, loss_sum, logits) if want_logits else (totals, loss_sum)


# ---- the tail of an evaluation pass over node batches: the same sums over selected rows (sgx_node_eval) ---------------------
def node_eval(H, weight, bias, target, totals, loss_sum, mask=None, n_prefix=None, want_logits=False):
    """The Linear head, the arg-max's hits and the summed cross entropy of the SELECTED rows of H, ADDED to accumulators
    that stay on the device, in one call (sgx_node_eval; the rule is in include/sgx.h, "the node evaluation head").
    H [n, P] fp32, weight [C, P] fp32, bias [C] fp32 or None, target [n] int64; row i is selected iff i < n_prefix (default
    n) and mask[i] (a bool or uint8 tensor [n], passed as its bytes; None: every row), node_loss's selection; the logits
    are node_loss's at p = 0 bit for bit.  totals: a device int64 [2] that receives += (selected rows, hits); loss_sum: a
    device float64 [1] that receives += the rows' losses (train.EvalSums holds such a pair).  Returns (totals, loss_sum),
    and the logits [n, C] of every row behind them with want_logits.  Never synchronises."""
    H, w, b = _loss_operands("node_eval", "H", H, weight, bias, target, None)
    (n, P), C = H.shape, w.shape[0]
    mask, n_prefix = _row_selection(mask, n_prefix, n)
    if n_prefix < 0:
        raise ValueError(f"node_eval: n_prefix = {n_prefix} is negative")
    _eval_accumulators("node_eval", totals, loss_sum)
    logits = torch.empty((n, C), dtype=torch.float32, device=H.device) if want_logits else None
    ws = _tail_workspace(H.device, lib.sgx_node_eval_workspace_bytes(n, n_prefix, P, C))
    check(lib.sgx_node_eval(n, n_prefix, P, C, _ptr(H), _ptr(w), _ptr(b), _ptr(target), _ptr(mask), _ptr(totals), _ptr(loss_sum),
                            _ptr(logits), *ws, _stream()),
          "sgx_node_eval")
    return (totals, loss_sum, logits) if want_logits else (totals, loss_sum)
