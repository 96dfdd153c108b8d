// GAT layers in the small-graph stack (sgx_gat_stack_forward): stack.hip's one launch per batch, with the edge softmax of
// sgx_gat_aggregate (one head, dead rows give 0) as a layer's aggregate.
//
// The kernel is gcn_stack_kernel's -- one 256-thread workgroup per plan group, the XD / Hs tiles, the same X.W, GCN
// aggregate and readout stages (stack_device.h) -- and a layer with gat_mode = 1 replaces the aggregate by three steps on
// the H tile in LDS:
//   1. s1_i = H_i.a1, s2_i = H_i.a2 for the group's rows: eight lanes per row, each an fp32 fma chain over the columns
//      t, t + 8, ..., added by an xor butterfly;
//   2. per row the maximum m_i of the live scores and 1 / sum of exp(x - m_i): eight lanes per row over the row's stored
//      entries, butterflies again;
//   3. D_i = act(sum_e w_e H_c), w_e = exp(x_e - m_i) / l_i: a group of lanes per row, one lane per four columns; the
//      lanes form the weights of as many entries as the group has lanes, one entry each (an exponential per entry, not
//      per entry and column chunk), and hand them round with a shuffle.
// The four fp32 arrays s1, s2, m, 1/l [rows] lie in LDS behind the two tiles.  No entry leaves the group, so nothing is
// exchanged with another workgroup; every sum has a fixed order that does not depend on the grid or on the grouping
// (a row's lanes and their order depend on the layer's width alone).  The stage and the kernel are in stack_gat_device.h.
#include "stack_gat_device.h"

namespace {

int check_gat_stack(const sgx_gat_stack_desc *d)
{
    return check_stack_desc(d, [](const sgx_gat_stack_layer &L) { return check_gat_layer(L); });
}

// the chained path's scratch beside H, D and W: the largest sgx_gat_scratch_bytes of the GAT layers
ChainCarve gat_chain_carve(const sgx_gat_stack_desc *d)
{
    size_t extra = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        if (!d->layer[l].gat_mode) continue;
        const size_t b = sgx_gat_scratch_bytes(d->n_rows, d->layer[l].P_w, 1, 0, nullptr);
        extra = b > extra ? b : extra;
    }
    return stack_chain_carve(d, extra);
}

int run_gat_chain(const sgx_gat_stack_desc *d, hipStream_t s)
{
    const ChainCarve c = gat_chain_carve(d);
    return stack_run_chain(d, c, s, [&](int l, const void *H, int64_t ldh, void *D, int64_t ldd) {
        const sgx_gat_stack_layer &L = d->layer[l];
        if (!L.gat_mode) return stack_chain_gcn(d, l, H, ldh, D, ldd, s);
        float *scratch = reinterpret_cast<float *>(static_cast<char *>(d->workspace) + c.x_off);
        return sgx_gat_aggregate(d->dtype, L.relu ? 1 : 0, /*fill_dead_rows*/0, d->n_rows, d->n_rows, L.P_w, 1, L.alpha,
                                 d->rowPtr_adj, d->columnIndex_adj, d->values_adj, H, ldh, L.attention, D, ldd, nullptr, nullptr,
                                 nullptr, scratch, s);
    });
}

int run_gat_fused(const sgx_gat_stack_desc *d, hipStream_t s)
{
    size_t lds;
    const GatStackArgs g = gat_stack_args(d, &lds);
    static sgx_lds_optin optin_f16, optin_f32;            // per kernel
    return d->dtype == SGX_F16 ? launch_stack_kernel(gat_stack_kernel<f16>, optin_f16, g, d->plan->n_groups, lds, s)
                               : launch_stack_kernel(gat_stack_kernel<float>, optin_f32, g, d->plan->n_groups, lds, s);
}

}  // namespace

extern "C" size_t sgx_gat_stack_workspace_bytes(const sgx_gat_stack_desc *d)
{
    if (check_gat_stack(d) != SGX_OK) return 0;
    if (d->n_rows == 0 && d->n_graphs == 0) return 0;              // nothing runs
    if (stack_fused_applies(d)) return 0;
    return gat_chain_carve(d).total;
}

extern "C" int sgx_gat_stack_forward(const sgx_gat_stack_desc *d, void *stream)
{
    const int rc = check_gat_stack(d);
    if (rc != SGX_OK) return rc;
    if (d->n_rows == 0 && d->n_graphs == 0) return SGX_OK;
    hipStream_t s = (hipStream_t)stream;
    return stack_fused_applies(d) ? run_gat_fused(d, s) : run_gat_chain(d, s);
}
