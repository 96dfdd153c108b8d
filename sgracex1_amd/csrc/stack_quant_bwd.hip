// Training the quantised small-graph stack (sgx_quant_stack_backward): stack_gat_bwd_device.h's one launch plus the
// reduction with a layer's quantiser (sgx_quant) in the forward quantities a GAT layer forms again.  The rule is
// FPYNQ_GAT.backward's under fake quantisation: the attention matrix is the quantised forward's S, and everything a
// gradient multiplies with is unquantised -- X_l, W_l, Wh = X_l . W_l and, in a GCN layer, the adjacency; deq_factor
// reaches no gradient (straight-through).
//
// Where the quantiser sits (StackQuantGrad; one fake_quantize_value / sgx_requant_value each, as in stack_quant.hip):
//   H_q        X_l on layer l's unsigned grid and W_l on the signed grid as the operands are fetched, the shift, clip
//              and decimal rounding on the store -- only to form s1, s2, m and 1 / l;
//   attention  signed grid, as the score pass reads it;
//   the mask   on the quantised adjacency value: values_adj_q as stored (SGX_QUANT_ADJ_DONE) or values_adj quantised as
//              it is read.
// Wh is then formed again from the unquantised operands over the same LDS tile.  A layer without a quantiser, and every
// GCN layer, runs sgx_gat_stack_backward's code.  Parity of the quantised layer is unpinned.
#include "stack_gat_bwd_device.h"

namespace {

// the quantisers' own errors come first (they need only the layer count), then sgx_gat_stack_backward's
int check_quant_grad(const sgx_quant_stack_grad_desc *d)
{
    if (!d) return SGX_ERR_NULL;
    if (d->n_layers < 1 || d->n_layers > kMaxLayers) return SGX_ERR_SHAPE;
    for (int l = 0; l < d->n_layers; ++l) {
        const sgx_quant_stack_grad_layer &L = d->layer[l];
        const sgx_quant *q = L.quant;
        if (!q) continue;
        if (d->dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;                               // SG.py:1545: float32 buffers
        if (q->qbits != 8 && q->qbits != 4 && q->qbits != 2 && q->qbits != 1) return SGX_ERR_UNSUPPORTED;
        if (q->scale_fea < 0 || q->scale_fea > 30 || q->internal_bits < 1 || q->internal_bits > 30) return SGX_ERR_UNSUPPORTED;
        // entries that are not stored must stay zero after quantisation, as in sgx_quant_stack_forward
        if (q->zero_adj != 0.0f || (L.gemm_mode == 0 && q->zero_fea != 0.0f)) return SGX_ERR_UNSUPPORTED;
        if (L.gat_mode == 1 && (q->flags & SGX_QUANT_ADJ_DONE) && !d->values_adj_q && d->n_rows > 0) return SGX_ERR_NULL;
    }
    return check_gat_grad(d);
}

bool any_quant_gat(const sgx_quant_stack_grad_desc *d)
{
    for (int l = 0; l < d->n_layers; ++l)
        if (d->layer[l].quant && d->layer[l].gat_mode == 1) return true;
    return false;
}

// the descriptor without its quantisers: sgx_gat_stack_backward's
sgx_gat_stack_grad_desc plain_grad_desc(const sgx_quant_stack_grad_desc *d)
{
    sgx_gat_stack_grad_desc g;
    g.dtype = d->dtype; g.n_layers = d->n_layers; g.n_rows = d->n_rows; g.n_graphs = d->n_graphs;
    g.graph_ptr = d->graph_ptr;
    g.rowPtr_adj = d->rowPtr_adj; g.columnIndex_adj = d->columnIndex_adj; g.values_adj = d->values_adj;
    g.rowPtr_fea = d->rowPtr_fea; g.columnIndex_fea = d->columnIndex_fea; g.values_fea = d->values_fea;
    for (int l = 0; l < kMaxLayers; ++l) {
        const sgx_quant_stack_grad_layer &L = d->layer[l];
        g.layer[l] = sgx_gat_stack_grad_layer{L.gemm_mode, L.relu, L.M_fea, L.P_w, L.W, L.D, L.ldd, L.grad_W, L.G, L.gat_mode,
                                              L.attention, L.alpha, L.grad_attention, L.S, L.E};
    }
    g.grad_pooled = d->grad_pooled;
    g.plan = d->plan; g.workspace = d->workspace; g.workspace_bytes = d->workspace_bytes;
    return g;
}

int launch_quant_backward(const sgx_quant_stack_grad_desc *d, const GatGradArgs &a, int grid, size_t lds, hipStream_t s)
{
    static sgx_lds_optin optin;
    StackQuantGrad sq = {};
    for (int l = 0; l < d->n_layers; ++l) {
        const sgx_quant *q = d->layer[l].quant;
        if (!q || d->layer[l].gat_mode != 1) continue;
        sq.on[l] = 1;
        sq.qbits[l] = q->qbits;
        sq.adj_done[l] = (q->flags & SGX_QUANT_ADJ_DONE) ? 1 : 0;
        sq.inv_fea[l] = q->inv_scale_fea; sq.zero_fea[l] = q->zero_fea;
        sq.inv_w[l] = q->inv_scale_w; sq.zero_w[l] = q->zero_w;
        sq.inv_adj[l] = q->inv_scale_adj; sq.zero_adj[l] = q->zero_adj;
        sq.ep_h[l] = sgx_requant_epilogue(q->scale_fea, q->internal_bits);
        sq.ep_d[l] = sgx_no_epilogue();                                   // (deq_factor reaches no gradient)
    }
    sq.val_q = static_cast<const float *>(d->values_adj_q);
    return launch_gat_backward(quant_stack_backward_kernel<float>, optin, a, grid, lds, s, sq);
}

}  // namespace

extern "C" size_t sgx_quant_stack_backward_lds_bytes(const sgx_quant_stack_grad_desc *d)
{
    if (check_quant_grad(d) != SGX_OK || gat_grad_supported(d) != SGX_OK) return 0;
    return gat_grad_lds(d->dtype, d->plan->max_width, d->plan->rows);
}

extern "C" size_t sgx_quant_stack_backward_workspace_bytes(const sgx_quant_stack_grad_desc *d)
{
    if (check_quant_grad(d) != SGX_OK || gat_grad_supported(d) != SGX_OK) return 0;
    return gat_grad_workspace(d);
}

extern "C" int sgx_quant_stack_backward(const sgx_quant_stack_grad_desc *d, void *stream)
{
    int rc = check_quant_grad(d);
    if (rc != SGX_OK) return rc;
    // a GCN layer's backward has no quantised step: without a quantised GAT layer the plain call is the call
    if (!any_quant_gat(d)) {
        const sgx_gat_stack_grad_desc g = plain_grad_desc(d);
        return sgx_gat_stack_backward(&g, stream);
    }
    rc = gat_grad_supported(d);
    if (rc != SGX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    return gat_backward_entry(d, s, [&](const GatGradArgs &a, int grid, size_t lds) { return launch_quant_backward(d, a, grid, lds, s); });
}
