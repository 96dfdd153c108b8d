"""Host side of jupyter/molecule_gcn/Graph_Classification.ipynb (MOL), same class names,
constructor and forward argument lists, with the FPGA offload replaced by the HIP kernels:

    RPYNQ, FPYNQ                 MOL cell 16   (torch.autograd.Function)
    Relu_pynq, GraphConvolution_pynq   MOL cell 17
    GraphConvolution             MOL cell 15   (the plain torch layer)
    GCN_PYNQ                     MOL cell 18

Differences that are forced by the platform, not by choice:
  * tensors live on the GPU; the eight `*_buffer` arguments of the forward calls are accepted
    and ignored when they are None (the reference stages CSR arrays through those PYNQ buffers;
    here the CSR arrays are handed to the kernel directly).  Passing real `pynq_shim` buffers
    still works and takes the register-map / AP_START path.
  * `adj` may be a dense tensor (as in the notebook, which builds a dense N x N matrix with
    to_dense_adj), a torch sparse CSR tensor, or an `ops.Csr`.
  * backward stays in torch on the device (the reference runs it in torch on the ARM CPU),
    except the two `adj @ ...` products, which go through the aggregation kernel.  Like the
    reference it multiplies by `adj`, not `adj^T` (exact for the symmetric graphs it is used on).
"""
import math

import torch
import torch.nn.functional as F
from torch.nn import Linear
from torch.nn.modules.module import Module
from torch.nn.parameter import Parameter

from . import ops
from .pyg_lite import global_mean_pool, to_dense_adj

ACC_DTYPE = torch.float16          # MOL cell 11: every accelerator buffer is np.float16


def as_csr(adj, dtype):
    """Dense / torch-sparse / ops.Csr -> ops.Csr in `dtype` (MOL cell 18 `adj._to_sparse_csr()`)."""
    if isinstance(adj, ops.Csr):
        return adj.to(dtype)
    if adj.layout == torch.sparse_csr:
        return ops.Csr(adj.crow_indices().to(torch.int32).contiguous(), adj.col_indices().to(torch.int32).contiguous(),
                       adj.values().to(dtype).contiguous(), adj.shape[1])
    if adj.layout == torch.sparse_coo:
        adj = adj.to_dense()
    return ops.Csr.from_dense(adj, dtype)


def feature_csr(x, dtype):
    """CSR of a (dense) feature matrix, kept on the tensor while it is unchanged: node features are the same
    tensor in every epoch, and the conversion costs a device->host sync (plus, in backward, a transpose)."""
    return ops.cached_on(x, ("fea_csr", dtype), lambda: as_csr(x.detach(), dtype))


class RPYNQ(torch.autograd.Function):
    """MOL cell 16: identity forward (the ReLU already ran inside the layer), backward zeroes the
    gradient where the layer's output is exactly 0."""

    @staticmethod
    def forward(ctx, input):
        ctx.save_for_backward(input)
        return input.clone()

    @staticmethod
    def backward(ctx, grad_output):
        input, = ctx.saved_tensors
        grad_input = grad_output.clone()
        if grad_input.is_cuda and input.dtype in (torch.float16, torch.float32) and \
                grad_input.dtype in (torch.float16, torch.float32):
            ops.relu_mask_backward_(input.contiguous(), grad_input)
        else:
            grad_input[input == 0] = 0
        return grad_input


class FPYNQ(torch.autograd.Function):
    """MOL cell 16.  forward(ctx, my_ip, adj, input, weights) -> Tensor[N, P] in the accelerator's
    element type; backward -> (None, None, grad_input, grad_weights) with
    grad_W = input^T @ adj @ g and grad_x = adj @ g @ W^T."""

    @staticmethod
    def forward(ctx, my_ip, adj, input, weights):
        rm = my_ip.register_map
        dense = int(rm.gemm_mode)
        A = as_csr(adj, ACC_DTYPE)
        rm.N_adj, rm.M_adj = A.n_rows, A.n_rows                     # MOL cell 16: both = adj.shape[0]
        rm.M_fea, rm.P_w = input.shape[1], weights.shape[1]
        Wt = torch.transpose(weights, 0, 1).detach().to(ACC_DTYPE).contiguous()      # B_buffer <- W^T
        if dense:
            fea = input.detach().to(ACC_DTYPE).contiguous()
        else:
            fea = feature_csr(input, ACC_DTYPE)
        output_acc = my_ip.run_layer(A, fea, Wt)
        ctx.adj = A
        ctx.fea_csr = None if dense else fea
        ctx.save_for_backward(input, weights, output_acc)
        return output_acc

    @staticmethod
    def backward(ctx, grad_output):
        """All three products on the device kernels, in fp32 as the reference's CPU backward:
        G = adj @ g (CSR aggregation), grad_W = X^T @ G (sgx_xt_g, or the aggregation kernel over
        the CSR of X^T when the layer's features were sparse), grad_x = G @ W^T (MFMA X.W kernel)."""
        input, weights, output = ctx.saved_tensors
        A = ctx.adj
        g = grad_output.float().contiguous()
        ag = ops.spmm(A.to(torch.float32), g)                                # adj @ g
        if ctx.fea_csr is not None:
            Xt = ctx.fea_csr.__dict__.get("_transposed")
            if Xt is None:
                Xt = ops.csr_transpose(ctx.fea_csr.to(torch.float32))
                ctx.fea_csr._transposed = Xt
            grad_weights = ops.spmm(Xt, ag)                                   # X^T @ (adj @ g)
        else:
            x = input if input.dtype in (torch.float16, torch.float32) else input.float()
            grad_weights = ops.xt_g(x.contiguous(), ag)
        grad_input = None
        if ctx.needs_input_grad[2]:
            grad_input = ops.xw_dense(ag, weights.detach().float().contiguous())   # (adj @ g) @ W^T
            if grad_input.stride(0) != grad_input.shape[1]:
                grad_input = grad_input.contiguous()
        return None, None, grad_input, grad_weights


class Relu_pynq(Module):
    def __init__(self):
        super(Relu_pynq, self).__init__()
        self.fn = RPYNQ.apply

    def forward(self, x):
        return self.fn(x)


class GraphConvolution(Module):
    """MOL cell 15: `adj @ input @ weight` in plain torch (bias optional)."""

    def __init__(self, in_features, out_features, bias=False):
        super(GraphConvolution, self).__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = Parameter(torch.FloatTensor(in_features, out_features))
        if bias:
            self.bias = Parameter(torch.FloatTensor(out_features))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)

    def forward(self, input, adj):
        output = adj @ input @ self.weight
        return output + self.bias if self.bias is not None else output

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class GraphConvolution_pynq(Module):
    """MOL cell 17.  The bias parameter exists and is never added, as in the reference."""

    def __init__(self, in_features, out_features, my_ip, bias=True):
        super(GraphConvolution_pynq, self).__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = Parameter(torch.FloatTensor(in_features, out_features))
        self.fn = FPYNQ.apply
        self.my_ip = my_ip
        if bias:
            self.bias = Parameter(torch.FloatTensor(out_features))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)

    def run_kernel(self):
        self.my_ip.register_map.CTRL.AP_START = 1
        kernel_done = self.my_ip.register_map.CTRL.AP_DONE
        while kernel_done == 0:
            kernel_done = self.my_ip.register_map.CTRL.AP_DONE

    def forward(self, acc, dense, relu, input, adj, rowPtr_fea_buffer=None, columnIndex_fea_buffer=None,
                values_fea_buffer=None, rowPtr_adj_buffer=None, columnIndex_adj_buffer=None,
                values_adj_buffer=None, B_buffer=None, D_buffer=None):
        if acc == 1:
            self.my_ip.register_map.relu = relu
            self.my_ip.register_map.gemm_mode = dense
            output = self.fn(self.my_ip, adj, input, self.weight)
        else:
            input = input.float()
            if isinstance(adj, ops.Csr):
                adj = torch.sparse_csr_tensor(adj.rowptr.long(), adj.col.long(), adj.val.float(),
                                              size=(adj.n_rows, adj.n_cols))
            output = adj @ input @ self.weight                       # the acc == 0 parity twin
        return output

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class GCN_PYNQ(torch.nn.Module):
    """MOL cell 18: conv1 (sparse X, ReLU in the kernel) -> Relu_pynq -> conv2 (dense X) ->
    global_mean_pool -> dropout(0.5) -> Linear.

    train_stack (opt-in, also settable as an attribute): with register layer_count >= 2, a training step's two layers
    and the pooling run as one forward and one backward call (ops.GcnStack) on a sorted, block-diagonal batch whose
    graphs fit the backward plan; every other case runs the layers one by one as before."""

    def __init__(self, hidden_channels, num_node_features, num_classes, my_ip, train_stack=False):
        super(GCN_PYNQ, self).__init__()
        self.train_stack = bool(train_stack)
        torch.manual_seed(12345)
        self.conv1 = GraphConvolution_pynq(num_node_features, hidden_channels, my_ip)
        self.conv2 = GraphConvolution_pynq(hidden_channels, hidden_channels, my_ip)
        self.reluh = Relu_pynq()
        self.lin = Linear(hidden_channels, num_classes)

    def forward(self, acc, x, edge_index, batch, rowPtr_fea_buffer=None, columnIndex_fea_buffer=None,
                values_fea_buffer=None, rowPtr_adj_buffer=None, columnIndex_adj_buffer=None,
                values_adj_buffer=None, B_buffer=None, D_buffer=None):
        bufs = (rowPtr_fea_buffer, columnIndex_fea_buffer, values_fea_buffer, rowPtr_adj_buffer,
                columnIndex_adj_buffer, values_adj_buffer, B_buffer, D_buffer)
        if acc == 1 and not self.training and not torch.is_grad_enabled() and self._stack_enabled():
            # layer_count >= 2 (the SGRACE register: layers per hardware call): the whole eval forward in one call
            out = self._forward_stack(x, edge_index, batch)
            if out is not None:
                return out
        if acc == 1 and getattr(self, "train_stack", False) and torch.is_grad_enabled() and self._stack_enabled():
            # the training step's GCN part as one forward and one backward call
            pooled = self._train_stack(x, edge_index, batch)
            if pooled is not None:
                x = F.dropout(pooled, p=0.5, training=self.training)
                return self.lin(x)
        x, ptr = self._layers(acc, x, edge_index, batch, bufs)
        if ptr is not None and not self.training and not torch.is_grad_enabled():
            # inference: pooling and the Linear head in one launch (dropout is the identity in eval)
            return ops.readout_mean_linear(x.contiguous(), ptr, self.lin.weight, self.lin.bias)
        if ptr is not None:
            # training: the pooling as one launch each way (the same fp32 means as the inference kernel); dropout and
            # the 64 x 2 head stay torch's here (train.StackTrainer runs them as one call, ops.head_loss)
            x = ops.ReadoutMean.apply(x, ptr, batch.numel() == x.shape[0])
        else:
            x = global_mean_pool(x.float(), batch)
        x = F.dropout(x, p=0.5, training=self.training)
        return self.lin(x)

    def _layers(self, acc, x, edge_index, batch, bufs=(None,) * 8):
        """The two layers one by one: (the second layer's output, graph_ptr of a sorted `batch` with acc = 1, else None)."""
        if acc == 1:
            # pynq_adj = to_dense_adj(edge_index)._to_sparse_csr() of the notebook, built from the
            # edge list directly (same CSR, no dense N x N intermediate); the batch of an epoch loop is
            # the same tensor every time, so the result is kept
            adj = ops.cached_on(edge_index, ("adj_csr", x.shape[0], ACC_DTYPE),
                                lambda: ops.csr_from_edge_index(edge_index, x.shape[0], dtype=ACC_DTYPE))
        else:
            adj = torch.squeeze(to_dense_adj(edge_index, num_nodes=x.shape[0]))
        dense, relu = 0, 1
        x = self.conv1(acc, dense, relu, x, adj, *bufs)
        x = x.relu() if acc == 0 else self.reluh(x)
        dense, relu = 1, 0
        x = self.conv2(acc, dense, relu, x, adj, *bufs)
        # a sorted `batch` (PyG's collation: graphs are contiguous) makes a graph a row segment; an unsorted one does not
        ptr = ops.graph_ptr_of(batch) if acc == 1 else None
        return x, ptr

    def layers_pooled(self, x, edge_index, batch):
        """The pooled means of the layer-by-layer training route on their own (acc = 1), for a caller that runs the tail
        itself on a batch train_pooled declines (train.StackTrainer): ops.ReadoutMean behind the two layers' autograd;
        None where `batch` is not sorted (the pooling is then torch's inside forward)."""
        h, ptr = self._layers(1, x, edge_index, batch)
        if ptr is None:
            return None
        return ops.ReadoutMean.apply(h, ptr, batch.numel() == h.shape[0])

    def _stack_enabled(self):
        """The register layer_count (the SGRACE register: layers per hardware call) asks for both layers in one call."""
        return getattr(self.conv1.my_ip.register_map, "layer_count", 1) >= 2

    def _stack_operands(self, x, edge_index, batch, backward):
        """What both stack routes need of a batch: (graph_ptr, the cached adjacency, the plan -- an SGX_BATCH_BACKWARD one
        that fits with `backward`, else the forward plan), or None when `batch` is not sorted, an edge joins two of its
        graphs or, with `backward`, a graph is over the plan's row budget or a width over its limit."""
        ptr = ops.graph_ptr_of(batch)
        if ptr is None:
            return None
        adj = ops.cached_on(edge_index, ("adj_csr", x.shape[0], ACC_DTYPE),
                            lambda: ops.csr_from_edge_index(edge_index, x.shape[0], dtype=ACC_DTYPE))
        width = max(self.conv1.out_features, self.conv2.in_features, self.conv2.out_features)
        if backward and width > 256:
            return None
        plan = ops.BatchPlan.cached(adj, ptr, width, ops._lib.SGX_BATCH_BACKWARD if backward else ops._lib.SGX_BATCH_FORWARD)
        if plan is None or (backward and not plan.fits):
            return None
        return ptr, adj, plan

    def _forward_stack(self, x, edge_index, batch, head=True):
        """Both layers, the mean pool and the head through ops.gcn_stack_forward: bit-equal to the layer-by-layer
        eval forward below, one launch for a batch of small graphs.  None (the caller then runs the layers one by one)
        when `batch` is not sorted or an edge joins two of its graphs.  head=False: the pooled means, without the head."""
        ready = self._stack_operands(x, edge_index, batch, backward=False)
        if ready is None:
            return None
        ptr, adj, plan = ready
        weights = [torch.transpose(c.weight, 0, 1).detach().to(ACC_DTYPE).contiguous() for c in (self.conv1, self.conv2)]
        return ops.gcn_stack_forward(adj, feature_csr(x, ACC_DTYPE), weights, [True, False], ptr, self.lin.weight if head else None,
                                     self.lin.bias if head else None, plan=plan)

    def eval_pooled(self, x, edge_index, batch):
        """The fused eval route up to the pooled means, for a caller that runs the tail itself (train.StackTrainer.evaluate):
        what forward(acc = 1, ...) pools in eval mode with gradients off where it takes the one call, None where it would
        not."""
        if self.training or torch.is_grad_enabled() or not self._stack_enabled():
            return None
        return self._forward_stack(x, edge_index, batch, head=False)

    def train_pooled(self, x, edge_index, batch):
        """The fused training route on its own, for a caller that runs the tail itself (train.StackTrainer): the pooled
        means behind ops.GcnStack where forward(acc = 1, ...) would take that route, None where it would not."""
        if not (getattr(self, "train_stack", False) and torch.is_grad_enabled() and self._stack_enabled()):
            return None
        return self._train_stack(x, edge_index, batch)

    def _train_stack(self, x, edge_index, batch):
        """Both layers and the mean pool through ops.GcnStack (one sgx_stack_forward, one sgx_stack_backward): the pooled
        means [G, hidden] fp32, bit-equal to the layer-by-layer forward.  None (the caller then runs the layers one by
        one) when x needs a gradient, `batch` is not sorted, an edge joins two of its graphs, a graph is over the
        backward plan's row budget or a width is over its limit."""
        ready = None if x.requires_grad else self._stack_operands(x, edge_index, batch, backward=True)
        if ready is None:
            return None
        ptr, adj, plan = ready
        return ops.GcnStack.apply(adj, feature_csr(x, ACC_DTYPE), ptr, plan, (True, False), self.conv1.weight,
                                  self.conv2.weight)
