// A batch of small graphs through the whole GCN stack in one launch (sgx_stack_forward; the reference's
// `layer_count` register, SG.py:1862).
//
// A sorted PyG batch makes graph g the row segment [graph_ptr[g], graph_ptr[g+1]) of a block-diagonal adjacency.
// The plan (sgx_batch_plan_create) checks that, and cuts the graphs into contiguous groups of at most R rows, R being
// what two [R][pitch] tiles of LDS hold.  One 256-thread workgroup per group then runs every stage in LDS:
//   X.W      layer 0: CSR feature rows against W^T in global (L2), or dense rows staged into LDS; layers >= 1 from the
//            previous D in LDS.  Dense products on the matrix cores, with the operand layout and K order of
//            xw_dense.hip, so H is bit-equal to sgx_xw_dense's.
//   A.H      one fp32 fma chain per (row, column) over the row's stored entries in CSR order (the sblock order of
//            spmm_csr.hip), columns rebased to the group's first row, gathers from LDS; D rounded and activated as
//            finish_value does, written back into LDS (and to the caller's D when asked).
//   readout  one wavefront per graph: the column means in row order, then the head's lane-strided fmas and the xor
//            butterfly of readout.hip -- the same bits as sgx_readout_mean_linear.
// Nothing crosses workgroups: no flags, no barriers beyond __syncthreads, no residency assumption.
//
// Where the plan does not fit (a graph over R rows) or a width is over the plan's, the same chain runs as separate
// launches through the workspace, with the same kernels as the layer path.
// The plan is built in stack_plan.hip; stack_bwd.hip trains the same stack (sgx_stack_backward).
#include "stack_device.h"

namespace {

template <typename T>
__global__ __launch_bounds__(kBlock) void gcn_stack_kernel(StackArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stack_lds[];
    T *const XD = reinterpret_cast<T *>(stack_lds);                 // X_l, then D_l      [rows][pitch]
    T *const Hs = XD + (size_t)a.rows * a.pitch;                    // H_l                [rows][pitch]
    const StackGroup grp = stack_group(a.group_graph, a.graph_ptr, a.rows, blockIdx.x);
    if (grp.gf >= grp.gl) return;
    const int r0 = grp.r0, nr = grp.nr;
    for (int l = 0; l < a.n_layers; ++l) {
        stack_form_h<T>(a, l, r0, nr, XD, Hs);
        __syncthreads();
        stack_gcn_aggregate<T>(a, l, r0, nr, XD, Hs);
        __syncthreads();
    }
    stack_readout<T>(a, grp.gf, grp.gl, r0, XD);
}

int check_stack(const sgx_stack_desc *d)
{
    return check_stack_desc(d, [](const sgx_stack_layer &) { return (int)SGX_OK; });
}

int run_chain(const sgx_stack_desc *d, hipStream_t s)
{
    return stack_run_chain(d, stack_chain_carve(d, 0), s, [&](int l, const void *H, int64_t ldh, void *D, int64_t ldd) {
        return stack_chain_gcn(d, l, H, ldh, D, ldd, s);
    });
}

int run_fused(const sgx_stack_desc *d, hipStream_t s)
{
    const sgx_batch_plan *p = d->plan;
    const StackArgs a = stack_args(d);
    const size_t lds = (size_t)2 * p->rows * a.pitch * sgx_elem_size(d->dtype);
    if (d->dtype == SGX_F16)
        hipLaunchKernelGGL(gcn_stack_kernel<f16>, dim3(p->n_groups), dim3(kBlock), lds, s, a);
    else
        hipLaunchKernelGGL(gcn_stack_kernel<float>, dim3(p->n_groups), dim3(kBlock), lds, s, a);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

}  // namespace

extern "C" size_t sgx_stack_workspace_bytes(const sgx_stack_desc *d)
{
    if (check_stack(d) != SGX_OK) return 0;
    if (stack_fused_applies(d)) return 0;
    return stack_chain_carve(d, 0).total;
}

extern "C" int sgx_stack_forward(const sgx_stack_desc *d, void *stream)
{
    const int rc = check_stack(d);
    if (rc != SGX_OK) return rc;
    if (d->n_rows == 0 && d->n_graphs == 0) return SGX_OK;
    hipStream_t s = (hipStream_t)stream;
    return stack_fused_applies(d) ? run_fused(d, s) : run_chain(d, s);
}
