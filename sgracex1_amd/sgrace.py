"""Host side of demo/sgrace_lib/sgrace.py (SG.py), same public names and signatures:

    sym_norm2                 SG.py:18-51
    RPYNQ                     SG.py:267-296
    FPYNQ_GAT                 SG.py:298-1126   forward(ctx, my_ip, self, adj, nnz_adj, input, weights,
                                               attention, out_features, dropout, relu)
    Relu_SGRACE               SG.py:1142-1162
    GATConv_SGRACE            SG.py:1164-1260  forward(compute_attention, dense, relu, input,
                                               edge_index, norm, adj)
    GAT_PYNQ                  demo/emulation/demo_sgrace.py:271-400 (the demo's two-layer model)
    GAT_POOL_PYNQ             demo/emulation/demo_sgrace.py:137-190 (the demo's graph classifier: the same two layers,
                                               global_mean_pool and a Linear head)
    init_SGRACE               SG.py:1271

`config.acc == 1` runs the layer on the GPU through the C ABI (GCN aggregate or single-head GAT
edge softmax, selected by `compute_attention` -> register gat_mode); `config.acc == 0` is the
reference's dense torch emulation (SG.py:563-681) kept as the parity twin.

Quantised bitstream (SG.py:53-265, :570-667, :1645-1848): with `config.w_qbits` in {8, 4, 2, 1} and
`config.fake_quantization == 1` (or `config.hardware_quantize == 1`), `init_SGRACE` derives the
constants (quant.py) and the layer runs with the quantised arithmetic -- on the GPU kernels for
`acc == 1` (the registers scale_fea, deq_factor, quantization_scale_*, quantized_multiplier are
programmed as the reference does, alternating between the layer-1 and layer-2 sets), in the dense
emulation for `acc == 0`.  The backward pass uses the unquantised operands, as in the reference.

Backward mirrors SG.py:884-1126 (the `accb == 0` branch) on the edge list instead of dense
N x N matrices: grad_input = P @ (g @ W^T), grad_weights = X^T @ (P @ g) with P = the attention
matrix (GAT) or adj (GCN) -- like the reference, P and not P^T -- and for GAT the attention-vector
gradient through softmax and LeakyReLU.  A GAT row without a positive entry in the adjacency the forward masked
with (the quantised one in quantised mode) has P = 1/N on all N columns, not only on its stored entries.

`config.accb == 1` (with `config.acc == 1`) runs that backward as ONE call of the C ABI, sgx_layer_backward: the same
arithmetic on the same kernels, the attention gradient gathered in row order instead of through a transposed pattern, a
CSR feature matrix never made dense, and grad_input left out when the input needs no gradient.  A flat-marked adjacency
(Csr.with_facts(flat=True)) of an unquantised layer takes that call's entry-split schedules (SGX_SCHEDULE_FLAT per matrix,
the attention gradient by stored entries): no plan, no read-back, so the step records and replays on padded batches of
any fan-out; with a quantiser the forward runs as without the fact, and so does the backward -- unless the adjacency also
carries flat_quant (Csr.with_facts(flat=True, flat_quant=True), as NeighborLoader(flat_quant=True) delivers it): the quantised
forward then takes the entry-split schedule (SGX_QUANT_FLAT) under config.accb = 0, whose staged backward already follows the
flat fact; the one-call backward of a quantised layer keeps the row schedule.
"""
import torch
import torch.nn.functional as F
from torch.nn import LeakyReLU, init
from torch.nn.modules.module import Module
from torch.nn.parameter import Parameter

import numpy as np

from . import config, ops, quant
from .molecule_gcn import RPYNQ  # noqa: F401  (same Function in both reference files)
from .pyg_lite import add_remaining_self_loops, global_mean_pool, sort_edge_index

my_ip = None
quant_constants = None        # set by init_SGRACE when the quantised path is selected
layern = 1                    # SG.py:327-359: the hardware path alternates two constant sets


def _quantised():
    return bool(config.fake_quantization) or bool(config.hardware_quantize)


def _f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32).item()


def _program_quant_registers(rm, qc):
    """SG.py:334-365, :476: what FPYNQ_GAT.forward writes before AP_START."""
    rm.scale_fea = qc.scale_fea
    rm.deq_factor = _f32_bits(qc.deq_o)
    rm.quantization_scale_fea = _f32_bits(1 / qc.f_s)
    rm.quantization_scale_w = _f32_bits(1 / qc.w_s)
    rm.quantization_scale_adj = _f32_bits(1 / qc.a_s)
    rm.quantized_multiplier = qc.internal_quantization


def _torch_dtype():
    import numpy as np
    return torch.float16 if np.dtype(config.float_type) == np.dtype(np.float16) else torch.float32


def sym_norm2(edge_index, num_nodes, edge_weight=None, fill=0, dtype=None):
    """SG.py:18-51: add the missing self loops with weight `fill`, sort by (row, col),
    D^-1/2 A D^-1/2 with D = row sums."""
    if edge_weight is None:
        edge_weight = torch.ones((edge_index.size(1),), dtype=dtype, device=edge_index.device)
    edge_index, edge_weight = add_remaining_self_loops(edge_index, edge_weight, fill, num_nodes)
    edge_index, edge_weight = sort_edge_index(edge_index, edge_weight, num_nodes)
    row, col = edge_index
    deg = torch.zeros(num_nodes, dtype=edge_weight.dtype, device=edge_weight.device).index_add_(0, row, edge_weight)
    deg_inv_sqrt = deg.pow(-0.5)
    deg_inv_sqrt[deg_inv_sqrt == float('inf')] = 0
    return edge_index, deg_inv_sqrt[row] * edge_weight * deg_inv_sqrt[col]


def _edge_csr(adj, edge_index, norm, n, dtype):
    """The CSR the kernel reads, from the (row-sorted) COO the reference ships (SG.py:1243-1247)."""
    if isinstance(adj, ops.Csr):
        return adj.to(dtype)
    row = edge_index[0].to(torch.int32).contiguous()
    return ops.Csr.from_coo(row, edge_index[1].to(torch.int32).contiguous(), norm.to(dtype).contiguous(), n, n)


def _fq_signed(x, s, z, qbits):
    """quantization_fbits (SG.py:238-251)."""
    t = 1 / s * x + z
    if qbits == 1:
        return torch.where(t < 0, torch.full_like(t, -0.5), torch.full_like(t, 0.5))
    lim = 2 ** (qbits - 1) - 1
    return torch.clip(torch.round(t), min=-lim, max=lim) / (2 ** (qbits - 1))


def _fq_unsigned(x, s, z, qbits):
    """quantization_ufbits (SG.py:253-265)."""
    q = torch.clip(torch.round(1 / s * x + z), min=0, max=2 ** qbits - 1)
    return q / 2 if qbits == 1 else q / (2 ** (qbits - 1))


def _lean_mask(ctx, A):
    """The values array the statistics form of the edge pass masks with (see FPYNQ_GAT.backward): the adjacency the forward
    masked with, or -- quantised, with dead rows -- that array with the dead rows' unquantised values; composed once."""
    M = ctx.masked
    if M is not A and ctx.dead is not None:
        if getattr(M, "_lean_values", None) is None:
            deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
            row = torch.repeat_interleave(torch.arange(A.n_rows, device=A.val.device), deg, output_size=A.nnz)
            M._lean_values = ops.Csr(A.rowptr, A.col, torch.where(ctx.dead[row], A.val[:A.nnz], M.val[:A.nnz]).contiguous(),
                                     A.n_cols)
        M = M._lean_values
    return M


class FPYNQ_GAT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, my_ip, self, adj, nnz_adj, input, weights, attention, out_features, dropout, relu):
        ctx.nheads, ctx.alpha, ctx.relu = self.nheads, self.alpha, relu
        ctx.gat = int(config.compute_attention)
        qc = None
        if _quantised():
            if quant_constants is None:
                raise RuntimeError("config.fake_quantization is set: call init_SGRACE() with config.w_qbits in {8, 4, 2, 1}")
            qc = quant_constants
        if config.acc == 1:
            dt = _torch_dtype()
            if qc is not None:
                global layern
                if dt != torch.float32:
                    raise TypeError("the quantised layer works on float32 buffers (SG.py:1545)")
                if layern == 2:
                    qc = qc.second_layer()
                layern = 2 if layern == 1 else 1
                _program_quant_registers(my_ip.register_map, qc)
            rm = my_ip.register_map
            A = self._csr.to(dt)
            Wt = weights.detach().t().to(dt).contiguous()
            fea = input.detach()
            if int(rm.gemm_mode) == 0:
                # the CSR of a feature matrix is rebuilt only when the tensor changes (node features are fixed
                # over the epochs of a node-classification run)
                fea = ops.cached_on(input, ("fea_csr", dt), lambda: ops.Csr.from_dense(
                    fea if fea.layout == torch.strided else fea.to_dense(), dt))
            else:
                fea = fea.to(dt).contiguous()
            # config.accb = 1: the backward as one call (sgx_layer_backward); its fp32 CSRs of X and X^T are built here,
            # once per feature tensor, so that the backward itself builds nothing
            ctx.accb, ctx.gemm_mode = int(config.accb), int(rm.gemm_mode)
            # a flat-marked adjacency: the one-call backward runs entry-split exactly where this forward does (unquantised)
            ctx.bwd_schedule = None if qc is None else "rows"
            if ctx.accb == 1 and ctx.gemm_mode == 0:
                ctx.fea32 = ops.feature_csr32(input)
            my_ip.alpha = self.alpha
            # config.hardware_quantize: the bitstream's own quantiser -- integer operands on the int8 matrix cores where
            # they are the faster form (dense features wider than 128 columns; sgx.h SGX_QUANT_INT8_AUTO);
            # config.fake_quantization alone: the fp32 emulation of the grid, as the reference states it
            int8 = "auto" if (qc is not None and config.hardware_quantize) else False
            # a flat-marked adjacency runs the entry-split aggregate, which writes no E / S: the statistics route whatever
            # config.gat_edge_outputs says.  The quantised layer takes that aggregate only for an adjacency that also carries
            # flat_quant (Csr.with_facts; ops.layer_forward reads the same two facts) and runs as without the fact otherwise
            ctx.lean = bool(ctx.gat) and (not int(config.gat_edge_outputs) or (A._flat and (qc is None or A._flat_quant)))
            if ctx.lean:
                # the row softmax statistics instead of E and S (3 n + n_cols floats in place of 2 nnz); the forward is
                # the one without side outputs
                out, stats = my_ip.run_layer(A, fea, Wt, attention=attention.detach().to(dt).reshape(-1).contiguous(),
                                             quant=qc, quant_int8=int8, want_row_stats=True)
            elif ctx.gat:
                out, E, S = my_ip.run_layer(A, fea, Wt, attention=attention.detach().to(dt).reshape(-1).contiguous(),
                                            want_edge_outputs=True, quant=qc, quant_int8=int8)
            else:
                out, E, S = my_ip.run_layer(A, fea, Wt, quant=qc, quant_int8=int8), None, None
            ctx.csr = A
            # the rows the forward gave a uniform softmax over all N columns: decided on the adjacency it masked with,
            # the quantised one when qc is set (ops.layer_forward); the mask is built once per graph
            ctx.dead = None
            if ctx.gat:
                masked = A.quantized(qc) if qc is not None else A
                ctx.dead = masked.dead_rows if masked.has_dead_rows else None
            if ctx.lean:
                ctx.masked = masked           # the adjacency the forward masked with: E and S are formed again on it
                ctx.save_for_backward(input, weights, out, *stats.tensors())
                return out.float()
            ctx.save_for_backward(input, weights, out, *([E, S] if ctx.gat else []))
            return out.float()                                            # SG.py:543 `.float()`

        # ---- no accelerator: the dense emulation of SG.py:563-681 --------------------------------
        input = input.float()
        input_q, weights_q, adj_d = input, weights, adj.to_dense()
        if qc is not None:                                                # SG.py:570-626
            input_q = _fq_unsigned(input, qc.f_s, qc.f_z, qc.w_qbits)
            weights_q = _fq_signed(weights, qc.w_s, qc.w_z, qc.w_qbits)
        Wh = torch.mm(input_q, weights_q)
        if qc is not None:
            iq = qc.internal_quantization
            Wh = Wh / (2 ** qc.scale_fea)
            Wh = torch.clip(Wh, min=-(2 ** iq - 1) / (2 ** iq), max=(2 ** iq - 1) / (2 ** iq))
            Wh = torch.round(Wh, decimals=iq - 1)
            attention = _fq_signed(attention, qc.w_s, qc.w_z, qc.w_qbits)
            adj_d = _fq_unsigned(adj_d, qc.a_s, qc.a_z, qc.w_qbits)
        Wh1 = torch.matmul(Wh, attention[:out_features, :])
        Wh2 = torch.matmul(Wh, attention[out_features:, :])
        e = self.leakyrelu(Wh1 + Wh2.T)
        attention1 = torch.where(adj_d > 0, e, -9e15 * torch.ones_like(e))
        attentions = F.softmax(attention1, dim=1)
        if ctx.gat:
            output_cpu = torch.matmul(attentions, Wh)
        else:
            # the sparse product, as SG.py does it: the dense one sums in another order on some CPUs (MKL's code path
            # depends on the instruction set), so only this form gives the reference's bits everywhere
            output_cpu = torch.matmul(adj_d.to_sparse(), Wh)
        if relu == 1:
            output_cpu = torch.where(output_cpu > 0, output_cpu, torch.zeros_like(output_cpu))
        if qc is not None:
            output_cpu = output_cpu * qc.deq_o                            # SG.py:666-667
        ctx.csr = None
        # SG.py:678-680 keep the UNquantised adjacency for the backward: P of the GCN form and the mask `adj > 0`
        adj_u = adj.to_dense().float()
        ctx.save_for_backward(input, weights, output_cpu, e, attentions if ctx.gat else adj_u, adj_u)
        return output_cpu

    @staticmethod
    def backward(ctx, grad_output):
        none = None
        g = grad_output.float()
        if ctx.csr is None:                                               # dense twin (SG.py:884-1126)
            input, weights, output, e, P, adj_d = ctx.saved_tensors
            Wh = input @ weights
            if ctx.gat:
                softmax_out = g @ Wh.t()
                dx = P * softmax_out
                sg = dx - P * dx.sum(dim=1, keepdim=True)
                sg = torch.where(adj_d > 0, sg, torch.zeros_like(sg))
                sg = ((e > 0) + ctx.alpha * (e <= 0)) * sg
                grad_attention = torch.cat([Wh.t() @ sg.sum(dim=1), (sg @ Wh).sum(dim=0)]).unsqueeze(1)
            else:
                grad_attention = torch.zeros((2 * weights.shape[1], 1), device=g.device)
            grad_input = P @ (g @ weights.t())
            grad_weights = input.t() @ (P @ g)
            return none, none, none, none, grad_input, grad_weights, grad_attention, none, none, none

        saved = ctx.saved_tensors
        if getattr(ctx, "accb", 0) == 1:
            # one call on the same kernels (include/sgx.h, sgx_layer_backward): no transposed pattern, a CSR X stays CSR,
            # grad_input only when the input wants it
            A, kw = ctx.csr, {}
            if ctx.gat:
                if ctx.lean:
                    kw = dict(stats=ops.GatStats.of(*saved[3:7]), mask=_lean_mask(ctx, A),
                              dead_weight=1.0 / A.n_cols if ctx.dead is not None else 0.0)
                else:
                    kw = dict(E=saved[3], S=saved[4])
                kw.update(dead=ctx.dead, alpha=ctx.alpha)
            X = ctx.fea32 if ctx.gemm_mode == 0 else saved[0].float().contiguous()
            grad_input, grad_weights, ga = ops.layer_backward(A, X, saved[1].float().contiguous(), g.contiguous(), gat=bool(ctx.gat),
                                                              gemm_mode=ctx.gemm_mode, want_grad_input=ctx.needs_input_grad[4],
                                                              schedule=ctx.bwd_schedule, **kw)
            if grad_input is not None and grad_input.stride(0) != grad_input.shape[1]:
                grad_input = grad_input.contiguous()
            grad_attention = ga.unsqueeze(1) if ctx.gat else torch.zeros((2 * saved[1].shape[1], 1), device=g.device)
            return none, none, none, none, grad_input, grad_weights, grad_attention, none, none, none
        input, weights, out = saved[0].float(), saved[1].float(), saved[2]
        if input.layout != torch.strided:
            input = input.to_dense()
        A = ctx.csr
        if ctx.gat:
            Wh = ops.xw_dense(input.contiguous(), weights.t().contiguous())       # X . W, fp32 (SG.py:601); rows padded to 16 B
            if getattr(ctx, "lean", False):
                # One values array decides both which entries carried weight in the forward and which the backward masks
                # (SG.py masks with the UNquantised adjacency).  Unquantised they are the same array.  Quantised, a live row
                # takes the quantised values (an entry that rounded to 0 had S = 0, so its sg is 0 under either mask) and a
                # dead row -- uniform weight whatever the values -- the unquantised ones, whose mask is the one that shows.
                M = _lean_mask(ctx, A)
                sg, g1, S = ops.gat_backward_edges_stats(M, ops.GatStats.of(*saved[3:7]), g.contiguous(), Wh, ctx.alpha,
                                                         dead=ctx.dead, dead_weight=1.0 / A.n_cols if ctx.dead is not None else 0.0)
            else:
                E, S = saved[3], saved[4]
                sg, g1 = ops.gat_backward_edges(A, E, S, g.contiguous(), Wh, ctx.alpha, dead=ctx.dead)
            # attention matrix, fp32 values; A's schedule -- and A's longest row where its builder knew it, so that P wants a
            # plan exactly where A does (a loader's batch of short rows builds none: no read-back, capturable)
            # -- and A's entry-split fact, so that P @ g takes the schedule A's own aggregate took
            P = ops.Csr(A.rowptr, A.col, S.contiguous(), A.n_cols, A.plan if A.wants_plan else None).with_facts(
                max_row=A._max_row, flat=A._flat)
            # column sums of sg = row sums over A^T; the transposed pattern is built once per graph
            if getattr(A, "_transpose_pattern", None) is None:
                A._transpose_pattern = ops.csr_transpose(A, return_order=True)
            AT, order = A._transpose_pattern
            ones = torch.ones((A.n_rows, 1), dtype=torch.float32, device=g.device)
            sgT = ops.Csr(AT.rowptr, AT.col, sg[order].contiguous(), AT.n_cols)
            # a hub column of A is a long row here: by stored entries for a flat-marked A (its transpose carries the fact),
            # one lane group per row otherwise
            g2 = ops.spmm(sgT.with_facts(flat=True), ones) if AT._flat else ops.spmm(sgT, ones, use_plan=False)
            ga = ops.xt_g(Wh, torch.cat([g1.unsqueeze(1), g2], dim=1).contiguous())   # [F, 2] = Wh^T [g1 g2]
            grad_attention = torch.cat([ga[:, 0], ga[:, 1]]).unsqueeze(1)
        else:
            P = A.to(torch.float32)
            grad_attention = torch.zeros((2 * weights.shape[1], 1), device=g.device)
        pg = ops.spmm(P, g.contiguous())                                       # P @ g
        if ctx.gat and ctx.dead is not None:                                   # a dead row of P is 1/N on every column
            pg = torch.where(ctx.dead.unsqueeze(1), (ops.col_sums(g.contiguous()) / A.n_cols).unsqueeze(0), pg)
        grad_input = ops.xw_dense(pg, weights.contiguous())                    # (P @ g) @ W^T == P @ (g @ W^T)
        if grad_input.stride(0) != grad_input.shape[1]:
            grad_input = grad_input.contiguous()
        grad_weights = ops.xt_g(input.contiguous(), pg)                        # X^T @ (P @ g)
        return none, none, none, none, grad_input, grad_weights, grad_attention, none, none, none


class Relu_SGRACE(Module):
    def __init__(self):
        super(Relu_SGRACE, self).__init__()
        self.fn = RPYNQ.apply

    def forward(self, x):
        return self.fn(x)


class GATConv_SGRACE(Module):
    """GAT / GCN layer of the SGRACE library.  `nheads` only widens W (single head, SG.py:1176-1178);
    the bias parameter exists and is never added, as in the reference."""

    def __init__(self, in_features, out_features, nheads=1, bias=True, dropout=0.2, alpha=0.2, concat=False):
        super(GATConv_SGRACE, self).__init__()
        self.in_features, self.out_features = in_features, out_features
        self.alpha, self.dropout = alpha, dropout
        self.weight = Parameter(torch.FloatTensor(in_features, out_features * nheads))
        init.xavier_uniform_(self.weight.data, gain=1.414)
        self.attention = Parameter(torch.empty(size=(2 * out_features * nheads, 1)))
        init.xavier_uniform_(self.attention.data, gain=1.414)
        self.leakyrelu = LeakyReLU(self.alpha)
        self.nheads, self.concat = nheads, concat
        self.fn = FPYNQ_GAT.apply
        self.my_ip = my_ip if config.acc == 1 else None
        self._csr = None
        if bias:
            self.bias = Parameter(torch.FloatTensor(out_features))
        else:
            self.register_parameter('bias', None)

    def run_kernel(self):
        self.my_ip.register_map.CTRL.AP_START = 1
        kernel_done = self.my_ip.register_map.CTRL.AP_DONE
        while kernel_done == 0:
            kernel_done = self.my_ip.register_map.CTRL.AP_DONE

    def forward(self, compute_attention, dense, relu, input, edge_index, norm, adj):
        nnz_adj = len(norm)
        if config.acc == 1:
            if self.my_ip is None:
                self.my_ip = my_ip
            if self.my_ip is None:
                raise RuntimeError("call init_SGRACE() before the first forward (config.acc == 1)")
            rm = self.my_ip.register_map
            rm.relu, rm.gemm_mode, rm.gat_mode = relu, dense, compute_attention
            rm.nnz_adj1 = nnz_adj
            # the CSR (with its row plan, quantised copy and dead-row check) is rebuilt only when the edge list
            # changes: the demo passes the same graph every epoch
            if isinstance(adj, ops.Csr):
                self._csr = adj.to(_torch_dtype())
            else:
                # kept on the edge list together with the `norm` it was built from (held, so that its identity
                # cannot be taken over by another tensor): rebuilt when either changes
                slot = ops.cached_on(edge_index, ("csr", input.shape[0], _torch_dtype()), dict)
                if slot.get("norm") is not norm or slot.get("norm_version") != norm._version:
                    slot.update(norm=norm, norm_version=norm._version,
                                csr=_edge_csr(None, edge_index, norm, input.shape[0], _torch_dtype()))
                self._csr = slot["csr"]
        return self.fn(self.my_ip, self, adj, nnz_adj, input, self.weight, self.attention, self.out_features,
                       self.dropout, relu)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class GAT_PYNQ(Module):
    """The two-layer model of the SGRACE demo (demo/emulation/demo_sgrace.py:271-400), same call pattern:
    sym_norm2 -> GATConv_SGRACE(compute_attention, dense=0, relu=1) -> Relu_SGRACE ->
    GATConv_SGRACE(dense=1, relu=0) -> dropout -> Linear.  The demo reads the feature / class counts from
    its global `dataset`; here they are constructor arguments."""

    def __init__(self, num_node_features, hidden_channels, head_count, num_classes):
        super(GAT_PYNQ, self).__init__()
        self.att2 = GATConv_SGRACE(num_node_features, hidden_channels, head_count, dropout=0.1, alpha=0.2, concat=False)
        self.conv22 = GATConv_SGRACE(hidden_channels * head_count, hidden_channels, 1)
        self.reluh = Relu_SGRACE()
        self.lin = torch.nn.Linear(hidden_channels, num_classes)

    def features(self, x, edge_index):
        """The two layers without the classifier tail: what dropout and self.lin receive, in fp32 (train.NodeTrainer runs
        that tail as one call, ops.node_loss)."""
        def normalise():                                          # once per graph, not per call
            ei, norm = sym_norm2(edge_index, x.size(0))
            adj = _edge_csr(None, ei, norm, x.size(0), _torch_dtype()) if config.acc == 1 else \
                torch.sparse_coo_tensor(ei, norm, (x.size(0), x.size(0)))
            return ei, norm, adj

        ei, norm, adj = ops.cached_on(edge_index, ("sym_norm2", x.size(0), config.acc, _torch_dtype()), normalise)
        x = self.att2(config.compute_attention, 0, 1, x, ei, norm, adj)
        x = self.reluh(x)
        x = self.conv22(config.compute_attention, 1, 0, x, ei, norm, adj)
        return x.float()

    def forward(self, x, edge_index):
        x = F.dropout(self.features(x, edge_index), p=0.5, training=self.training)
        return self.lin(x)


class GAT_POOL_PYNQ(Module):
    """The graph classifier of the SGRACE demo (demo/emulation/demo_sgrace.py:137-190) on a PyG batch of graphs:
    sym_norm2 -> GATConv_SGRACE(compute_attention, dense=0, relu=1) -> Relu_SGRACE -> GATConv_SGRACE(dense=1, relu=0) ->
    global_mean_pool -> dropout(0.5) -> Linear.  Training runs layer by layer through FPYNQ_GAT's autograd.

    With register layer_count >= 2 (layers per hardware call, SG.py:1862) the eval forward runs as ONE call,
    ops.gat_stack_forward (GCN layers in it when config.compute_attention == 0), where all of these hold: eval mode with
    gradients off, config.acc == 1, `batch` sorted with no edge between two of its graphs, and no row of the adjacency
    without a positive entry (the stack gives such a row 0, the layer the mean of all rows; sym_norm2's self loops leave
    none).  With the quantiser on (config.fake_quantization / hardware_quantize) the one call is
    ops.quant_stack_forward -- layer 1 on quant_constants, layer 2 on its second_layer(), the cached quantised adjacency,
    `layern` and the quantiser registers left as the two layer calls leave them -- where also config.float_type is
    float32, the dead-row condition holds on the QUANTISED adjacency (at 4 bits and below the quantiser can kill a row),
    and not both config.hardware_quantize and a hidden width over 128 (there the layer takes the int8 form, whose sums may
    round differently).  Parity of the quantised layers is unpinned, as everywhere: the reference records no quantised
    output.  Every other case runs the layers one by one.

    train_stack (opt-in, also settable as an attribute): with layer_count >= 2 a training step's two layers and the mean
    pool run as one forward and one backward call (ops.GatStack: sgx_gat_stack_forward, sgx_gat_stack_backward; GCN layers
    in them when config.compute_attention == 0) where all of these hold: config.acc == 1, x needing no gradient, `batch`
    sorted with no edge between two of its graphs, no row of the adjacency without a positive entry, one alpha for both
    layers, and every graph within the backward plan's row budget.  With the quantiser on the two calls are ops.QuantStack
    (sgx_quant_stack_forward, sgx_quant_stack_backward: the quantised forward's attention matrix, unquantised operands in
    every gradient, as FPYNQ_GAT.backward) under the quantised eval route's conditions as well -- float32,
    quant_constants set, the dead-row condition on the QUANTISED adjacency, not both config.hardware_quantize and a hidden
    width over 128 -- with `layern` and the quantiser registers left as the two layer calls leave them; parity unpinned.
    Dropout and the head stay in torch behind the pooled output.  Every other case runs the layers one by one."""

    def __init__(self, num_node_features, hidden_channels, num_classes, train_stack=False):
        super(GAT_POOL_PYNQ, self).__init__()
        self.train_stack = bool(train_stack)
        self.att1 = GATConv_SGRACE(num_node_features, hidden_channels, 1)
        self.att2 = GATConv_SGRACE(hidden_channels, hidden_channels, 1)
        self.reluh = Relu_SGRACE()
        self.lin = torch.nn.Linear(hidden_channels, num_classes)

    @staticmethod
    def _normalised(x, edge_index):
        def normalise():                                          # once per batch, not per call
            ei, norm = sym_norm2(edge_index, x.size(0))
            adj = _edge_csr(None, ei, norm, x.size(0), _torch_dtype()) if config.acc == 1 else \
                torch.sparse_coo_tensor(ei, norm, (x.size(0), x.size(0)))
            return ei, norm, adj

        return ops.cached_on(edge_index, ("sym_norm2", x.size(0), config.acc, _torch_dtype()), normalise)

    @staticmethod
    def _stack_enabled():
        """The kernels are on and the register layer_count asks for both layers in one call."""
        return config.acc == 1 and my_ip is not None and getattr(my_ip.register_map, "layer_count", 1) >= 2

    def train_pooled(self, x, edge_index, batch):
        """The fused training route on its own, for a caller that runs the tail itself (train.StackTrainer): the pooled
        means behind ops.GatStack / ops.QuantStack where forward would take that route, None where it would not."""
        if not (self._stack_enabled() and getattr(self, "train_stack", False) and torch.is_grad_enabled()):
            return None
        return self._train_stack(x, self._normalised(x, edge_index)[2], batch)

    def forward(self, x, edge_index, batch):
        ei, norm, adj = self._normalised(x, edge_index)
        if self._stack_enabled() and not self.training and not torch.is_grad_enabled():
            out = self._forward_stack(x, adj, batch)
            if out is not None:
                return out
        if self._stack_enabled() and getattr(self, "train_stack", False) and torch.is_grad_enabled():
            # the training step's two layers and the pooling as one forward and one backward call
            pooled = self._train_stack(x, adj, batch)
            if pooled is not None:
                return self.lin(F.dropout(pooled, p=0.5, training=self.training))
        x, ptr = self._layers(x, ei, norm, adj, batch)
        if ptr is not None and not self.training and not torch.is_grad_enabled():
            return ops.readout_mean_linear(x.contiguous(), ptr, self.lin.weight, self.lin.bias)
        if ptr is not None:
            x = ops.ReadoutMean.apply(x, ptr, batch.numel() == x.shape[0])
        else:
            x = global_mean_pool(x.float(), batch)
        x = F.dropout(x, p=0.5, training=self.training)
        return self.lin(x)

    def _layers(self, x, ei, norm, adj, batch):
        """The two layers one by one: (the second layer's output, graph_ptr of a sorted `batch` with acc = 1, else None)."""
        x = self.att1(config.compute_attention, 0, 1, x, ei, norm, adj)
        x = self.reluh(x)
        x = self.att2(config.compute_attention, 1, 0, x, ei, norm, adj)
        # a sorted `batch` makes a graph a row segment; an unsorted one does not
        ptr = ops.graph_ptr_of(batch) if config.acc == 1 else None
        return x, ptr

    def layers_pooled(self, x, edge_index, batch):
        """The pooled means of the layer-by-layer training route on their own, for a caller that runs the tail itself on a
        batch train_pooled declines (train.StackTrainer): ops.ReadoutMean behind the two layers' autograd; None where
        config.acc != 1 or `batch` is not sorted (the pooling is then torch's inside forward)."""
        if config.acc != 1:
            return None
        ei, norm, adj = self._normalised(x, edge_index)
        h, ptr = self._layers(x, ei, norm, adj, batch)
        if ptr is None:
            return None
        return ops.ReadoutMean.apply(h, ptr, batch.numel() == h.shape[0])

    def _stack_operands(self, x, adj, batch, backward):
        """What both stack routes need of a batch: (graph_ptr, the plan -- an SGX_BATCH_BACKWARD one that fits with
        `backward`, else the forward plan --, the feature CSR, the adjacency a GAT layer masks with, the two layers'
        quantisers or None), or None where one of the class docstring's conditions fails."""
        dt = _torch_dtype()
        ptr = ops.graph_ptr_of(batch)
        gat = int(config.compute_attention)
        qc = None
        if _quantised():
            qc = quant_constants
            # (no constants, fp16: the layer's own errors; int8 operands: the layer's own form)
            if qc is None or dt != torch.float32 or (config.hardware_quantize and self.att2.weight.shape[0] > 128):
                return None
        masked = adj if qc is None else adj.quantized(qc)
        if ptr is None or (gat and (self.att1.alpha != self.att2.alpha or masked.has_dead_rows is not False)):
            return None
        width = max(self.att1.weight.shape[1], self.att2.weight.shape[0], self.att2.weight.shape[1])
        if backward and width > 256:
            return None
        plan = ops.BatchPlan.cached(adj, ptr, width, ops._lib.SGX_BATCH_BACKWARD if backward else ops._lib.SGX_BATCH_FORWARD)
        if plan is None or (backward and not plan.fits):
            return None
        fea = ops.cached_on(x, ("fea_csr", dt), lambda: ops.Csr.from_dense(
            x.detach() if x.layout == torch.strided else x.detach().to_dense(), dt))
        # the constants of the two layer calls (FPYNQ_GAT.forward): `layern` alternates the two sets
        quants = None if qc is None else (qc.second_layer() if layern == 2 else qc, qc if layern == 2 else qc.second_layer())
        return ptr, plan, fea, masked, quants

    def eval_pooled(self, x, edge_index, batch):
        """The fused eval route up to the pooled means, for a caller that runs the tail itself (train.StackTrainer.evaluate):
        what forward pools in eval mode with gradients off where it takes the one call, None where it would not."""
        if self.training or torch.is_grad_enabled() or not self._stack_enabled():
            return None
        return self._forward_stack(x, self._normalised(x, edge_index)[2], batch, head=False)

    def _forward_stack(self, x, adj, batch, head=True):
        """Both layers, the mean pool and the head through ops.gat_stack_forward (ops.quant_stack_forward with the
        quantiser on); None (the caller then runs the layers one by one) where the stack does not compute what they do.
        head=False: the pooled means, without the head."""
        ready = self._stack_operands(x, adj, batch, backward=False)
        if ready is None:
            return None
        ptr, plan, fea, masked, quants = ready
        dt, gat, layers = _torch_dtype(), int(config.compute_attention), (self.att1, self.att2)
        weights = [c.weight.detach().t().to(dt).contiguous() for c in layers]
        atts = [c.attention.detach().to(dt).reshape(-1).contiguous() if gat else None for c in layers]
        lin_w, lin_b = (self.lin.weight, self.lin.bias) if head else (None, None)
        if quants is not None:
            _program_quant_registers(my_ip.register_map, quants[1])                # the registers of the two layer calls
            return ops.quant_stack_forward(masked, fea, weights, atts, [True, False], ptr, quants, lin_w, lin_b,
                                           alpha=self.att1.alpha, plan=plan, adj_quantised=True)
        return ops.gat_stack_forward(adj, fea, weights, atts, [True, False], ptr, lin_w, lin_b, alpha=self.att1.alpha, plan=plan)

    def _train_stack(self, x, adj, batch):
        """Both layers and the mean pool through ops.GatStack (ops.QuantStack with the quantiser on): the pooled means
        [G, hidden] fp32 with the gradients of the weights and the attention vectors behind them.  None (the caller then
        runs the layers one by one) where one of the class docstring's conditions fails."""
        ready = None if x.requires_grad else self._stack_operands(x, adj, batch, backward=True)
        if ready is None:
            return None
        ptr, plan, fea, masked, quants = ready
        layers = (self.att1, self.att2)
        atts = [c.attention if int(config.compute_attention) else None for c in layers]
        if quants is not None:
            _program_quant_registers(my_ip.register_map, quants[1])                # the registers of the two layer calls
            return ops.QuantStack.apply(adj, masked, fea, ptr, plan, (True, False), self.att1.alpha, quants,
                                        *[c.weight for c in layers], *atts)
        return ops.GatStack.apply(adj, fea, ptr, plan, (True, False), self.att1.alpha, *[c.weight for c in layers], *atts)


def init_SGRACE(device=None):
    """SG.py:1271: opens the overlay and publishes the IP handle the layers use."""
    global my_ip, quant_constants, layern
    layern = 1
    quant_constants = quant.constants(config.w_qbits) if _quantised() else None
    if config.acc == 1:
        from .pynq_shim import Overlay
        ol = Overlay("gat_all_unsigned.bit", device=device or config.device)
        my_ip = ol.mmult_top_0
        if quant_constants is not None:          # SG.py:1745-1839: f_align is the hardware's input alignment, unused here
            my_ip.register_map.beta_qu = {8: 255, 4: 15, 2: 2, 1: 1}[config.w_qbits]
            my_ip.register_map.f_align = {8: 0, 4: 4, 2: 6, 1: 7}[config.w_qbits]
    return my_ip
