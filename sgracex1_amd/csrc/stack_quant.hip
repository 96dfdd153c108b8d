// Quantised layers in the small-graph stack (sgx_quant_stack_forward): stack_gat.hip's one launch per batch with a
// layer's quantiser (sgx_quant) inside the stages -- what sgx_layer_forward does with four quantiser launches, two
// epilogues and a dozen kernels per layer, for a batch of molecules that fits a workgroup's LDS.
//
// Where each rounding point sits (StackQuant, stack_device.h; one fake_quantize_value / sgx_requant_value each, the
// statements sgx_fake_quantize and the layer's store epilogues are made of):
//   W, attention  signed grid, on the element as the MFMA operand load (or the sparse stage, or the score pass) reads it;
//   X_0           unsigned grid, on the CSR entry as it is read / on the dense row as it is copied into LDS;
//   X_l, l >= 1   unsigned grid of layer l, where layer l - 1's aggregate stores D_{l-1} into the X tile (the caller's D
//                 gets the unquantised value; the last tile is not quantised: the readout reads D);
//   A             unsigned grid, on the stored value as an aggregate reads it (not with SGX_QUANT_ADJ_DONE);
//   H             shift, clip, decimal rounding on the X.W store;
//   D             ReLU, then deq_factor, on the aggregate's store.
// Every operand is quantised exactly once -- the quantiser is not idempotent.  Parity of the quantised layer is unpinned
// (the reference records no quantised output); the tests pin equality with sgx_layer_forward.
#include "stack_gat_device.h"

namespace {

int check_quant(const sgx_quant_stack_desc *d, const sgx_quant_stack_layer &L)
{
    const sgx_quant *q = L.quant;
    if (!q) return SGX_OK;
    if (d->dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;                                   // SG.py:1545: float32 buffers
    if (q->qbits != 8 && q->qbits != 4 && q->qbits != 2 && q->qbits != 1) return SGX_ERR_UNSUPPORTED;
    if (q->scale_fea < 0 || q->scale_fea > 30 || q->internal_bits < 1 || q->internal_bits > 30) return SGX_ERR_UNSUPPORTED;
    // entries that are not stored must stay zero after quantisation, as in sgx_layer_forward
    if (q->zero_adj != 0.0f || (L.gemm_mode == 0 && q->zero_fea != 0.0f)) return SGX_ERR_UNSUPPORTED;
    return SGX_OK;
}

int check_quant_stack(const sgx_quant_stack_desc *d)
{
    // (d is not NULL inside the layer check: check_stack_desc returns before it)
    return check_stack_desc(d, [d](const sgx_quant_stack_layer &L) {
        const int rc = check_gat_layer(L);
        return rc != SGX_OK ? rc : check_quant(d, L);
    });
}

bool any_quant(const sgx_quant_stack_desc *d)
{
    for (int l = 0; l < d->n_layers; ++l)
        if (d->layer[l].quant) return true;
    return false;
}

// the descriptor without its quantisers (every one NULL): sgx_gat_stack_forward's
sgx_gat_stack_desc plain_desc(const sgx_quant_stack_desc *d)
{
    sgx_gat_stack_desc g;
    g.dtype = d->dtype; g.n_layers = d->n_layers; g.n_rows = d->n_rows; g.n_graphs = d->n_graphs;
    g.graph_ptr = d->graph_ptr;
    g.rowPtr_adj = d->rowPtr_adj; g.columnIndex_adj = d->columnIndex_adj; g.values_adj = d->values_adj;
    g.rowPtr_fea = d->rowPtr_fea; g.columnIndex_fea = d->columnIndex_fea; g.values_fea = d->values_fea;
    for (int l = 0; l < kMaxLayers; ++l) {
        const sgx_quant_stack_layer &L = d->layer[l];
        g.layer[l] = sgx_gat_stack_layer{L.gemm_mode, L.relu, L.M_fea, L.P_w, L.B, L.D, L.ldd, L.gat_mode, L.attention, L.alpha};
    }
    g.C = d->C; g.W_head = d->W_head; g.bias = d->bias; g.pooled = d->pooled; g.logits = d->logits;
    g.plan = d->plan; g.workspace = d->workspace; g.workspace_bytes = d->workspace_bytes;
    return g;
}

// ---- the chained path: sgx_layer_forward per layer, sgx_readout_mean_linear, through the workspace -------------------
// layer l's quantiser as the chain hands it on: the stack takes the fp32 form, so only SGX_QUANT_ADJ_DONE stays
sgx_quant chain_quant(const sgx_quant *q)
{
    sgx_quant c = *q;
    c.flags &= SGX_QUANT_ADJ_DONE;
    return c;
}

// layer l of the chain on input X [n_rows][M_fea] (or the caller's CSR), output D [n_rows][P_w]; q: storage for its quantiser
sgx_layer_desc chain_layer(const sgx_quant_stack_desc *d, int l, const void *X, void *D, sgx_quant *q)
{
    const sgx_quant_stack_layer &L = d->layer[l];
    sgx_layer_desc ld = {};
    ld.gemm_mode = L.gemm_mode; ld.relu = L.relu ? 1 : 0; ld.gat_mode = L.gat_mode;
    ld.N_adj = ld.M_adj = d->n_rows; ld.M_fea = L.M_fea; ld.P_w = L.P_w;
    ld.dtype = d->dtype; ld.acc_mode = SGX_ACC_F32; ld.spmm_block = 1; ld.gat_fill_dead_rows = 0;
    ld.B = L.B; ld.D = D;
    if (L.gemm_mode == 0) { ld.rowPtr_fea = d->rowPtr_fea; ld.columnIndex_fea = d->columnIndex_fea; }
    ld.values_fea = X;
    ld.rowPtr_adj = d->rowPtr_adj; ld.columnIndex_adj = d->columnIndex_adj; ld.values_adj = d->values_adj;
    ld.attention = L.gat_mode ? L.attention : nullptr; ld.alpha = L.alpha; ld.gat_heads = 1;
    ld.fea_threads = ld.adj_threads = 1;
    if (L.quant) { *q = chain_quant(L.quant); ld.quant = q; }
    ld.order = SGX_ORDER_REFERENCE;
    return ld;
}

struct QuantChainCarve {
    size_t d_off[2], l_off, l_bytes, total;    // two D buffers [n_rows][widest P_w], then the layers' own workspace
};

QuantChainCarve quant_chain_carve(const sgx_quant_stack_desc *d)
{
    QuantChainCarve c;
    const size_t es = sgx_elem_size(d->dtype);
    int pmax = 1;
    c.l_bytes = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        pmax = d->layer[l].P_w > pmax ? d->layer[l].P_w : pmax;
        sgx_quant q;
        const sgx_layer_desc ld = chain_layer(d, l, nullptr, nullptr, &q);
        const size_t b = sgx_layer_workspace_bytes(&ld);
        c.l_bytes = b > c.l_bytes ? b : c.l_bytes;
    }
    size_t off = 0;
    for (int i = 0; i < 2; ++i) { c.d_off[i] = off; off += sgx_align_up((size_t)d->n_rows * pmax * es, 256); }
    c.l_off = off; off += sgx_align_up(c.l_bytes, 256);
    c.total = off < 256 ? 256 : off;            // (never 0: 0 says "fused")
    return c;
}

int run_quant_chain(const sgx_quant_stack_desc *d, hipStream_t s)
{
    const QuantChainCarve c = quant_chain_carve(d);
    if (!d->workspace || d->workspace_bytes < c.total) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)d->workspace % 256 != 0) return SGX_ERR_ALIGN;
    char *ws = static_cast<char *>(d->workspace);
    const size_t es = sgx_elem_size(d->dtype);
    const void *X = d->values_fea;
    for (int l = 0; l < d->n_layers; ++l) {
        const sgx_quant_stack_layer &L = d->layer[l];
        // the layer writes D densely ([n_rows][P_w]): straight into the caller's D where that is its pitch
        const bool direct = L.D && layer_ldd(L) == L.P_w;
        void *D = direct ? L.D : ws + c.d_off[l & 1];
        sgx_quant q;
        sgx_layer_desc ld = chain_layer(d, l, X, D, &q);
        ld.workspace = ws + c.l_off;
        ld.workspace_bytes = c.l_bytes;
        const int rc = sgx_layer_forward(&ld, s);
        if (rc != SGX_OK) return rc;
        if (L.D && !direct && d->n_rows > 0)
            SGX_HIP_CHECK(hipMemcpy2DAsync(L.D, (size_t)layer_ldd(L) * es, D, (size_t)L.P_w * es, (size_t)L.P_w * es, d->n_rows,
                                           hipMemcpyDeviceToDevice, s));
        X = D;
    }
    float *logits = d->C > 0 ? d->logits : nullptr;
    if (!d->pooled && !logits) return SGX_OK;
    const int F = d->layer[d->n_layers - 1].P_w;
    return sgx_readout_mean_linear(d->dtype, d->n_graphs, F, logits ? d->C : 0, X, F, d->graph_ptr, d->W_head, d->bias,
                                   d->pooled, logits, s);
}

// ---- the fused path --------------------------------------------------------------------------------------------------
int run_quant_fused(const sgx_quant_stack_desc *d, hipStream_t s)
{
    size_t lds;
    const GatStackArgs g = gat_stack_args(d, &lds);
    StackQuant sq = {};
    for (int l = 0; l < d->n_layers; ++l) {
        const sgx_quant *q = d->layer[l].quant;
        if (!q) continue;
        sq.on[l] = 1;
        sq.qbits[l] = q->qbits;
        sq.adj_done[l] = (q->flags & SGX_QUANT_ADJ_DONE) ? 1 : 0;
        sq.inv_fea[l] = q->inv_scale_fea; sq.zero_fea[l] = q->zero_fea;
        sq.inv_w[l] = q->inv_scale_w; sq.zero_w[l] = q->zero_w;
        sq.inv_adj[l] = q->inv_scale_adj; sq.zero_adj[l] = q->zero_adj;
        sq.ep_h[l] = sgx_requant_epilogue(q->scale_fea, q->internal_bits);
        sq.ep_d[l] = sgx_no_epilogue();
        sq.ep_d[l].out_scale = q->deq_factor;
    }
    static sgx_lds_optin optin;
    return launch_stack_kernel(quant_stack_kernel<float>, optin, g, d->plan->n_groups, lds, s, sq);
}

}  // namespace

extern "C" size_t sgx_quant_stack_workspace_bytes(const sgx_quant_stack_desc *d)
{
    if (check_quant_stack(d) != SGX_OK) return 0;
    if (!any_quant(d)) {
        const sgx_gat_stack_desc g = plain_desc(d);
        return sgx_gat_stack_workspace_bytes(&g);
    }
    if (d->n_rows == 0 && d->n_graphs == 0) return 0;              // nothing runs
    if (stack_fused_applies(d)) return 0;
    return quant_chain_carve(d).total;
}

extern "C" int sgx_quant_stack_forward(const sgx_quant_stack_desc *d, void *stream)
{
    const int rc = check_quant_stack(d);
    if (rc != SGX_OK) return rc;
    if (!any_quant(d)) {
        const sgx_gat_stack_desc g = plain_desc(d);
        return sgx_gat_stack_forward(&g, stream);
    }
    if (d->n_rows == 0 && d->n_graphs == 0) return SGX_OK;
    hipStream_t s = (hipStream_t)stream;
    return stack_fused_applies(d) ? run_quant_fused(d, s) : run_quant_chain(d, s);
}
