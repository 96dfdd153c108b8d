// sgx_gat_stack_backward: the small-graph stack's backward with GAT layers (stack_gat_bwd_device.h) without a
// quantiser -- StackPlain compiles every hook of that body out.
#include "stack_gat_bwd_device.h"

namespace {

int launch_plain_backward(const sgx_gat_stack_grad_desc *d, const GatGradArgs &a, int grid, size_t lds, hipStream_t s)
{
    static sgx_lds_optin optin_f16, optin_f32;            // per instantiation
    return d->dtype == SGX_F16 ? launch_gat_backward(gat_stack_backward_kernel<f16>, optin_f16, a, grid, lds, s)
                               : launch_gat_backward(gat_stack_backward_kernel<float>, optin_f32, a, grid, lds, s);
}

}  // namespace

extern "C" size_t sgx_gat_stack_backward_lds_bytes(const sgx_gat_stack_grad_desc *d)
{
    if (check_gat_grad(d) != SGX_OK || gat_grad_supported(d) != SGX_OK) return 0;
    return gat_grad_lds(d->dtype, d->plan->max_width, d->plan->rows);
}

extern "C" size_t sgx_gat_stack_backward_workspace_bytes(const sgx_gat_stack_grad_desc *d)
{
    if (check_gat_grad(d) != SGX_OK || gat_grad_supported(d) != SGX_OK) return 0;
    return gat_grad_workspace(d);
}

extern "C" int sgx_gat_stack_backward(const sgx_gat_stack_grad_desc *d, void *stream)
{
    int rc = check_gat_grad(d);
    if (rc != SGX_OK) return rc;
    rc = gat_grad_supported(d);
    if (rc != SGX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    return gat_backward_entry(d, s, [&](const GatGradArgs &a, int grid, size_t lds) { return launch_plain_backward(d, a, grid, lds, s); });
}
