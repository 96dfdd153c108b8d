// The classifier tail of a training step in one call (sgx_head_loss, include/sgx.h "the loss head"): dropout on the
// pooled means, the C x P Linear head, softmax cross entropy (mean over the graphs) and every gradient of it --
// grad_pooled for the stack's backward, grad_W / grad_bias for the optimiser.  What GCN_PYNQ / GAT_POOL_PYNQ run as
// F.dropout, self.lin, CrossEntropyLoss and their autograd nodes.
//
// One workgroup per graph slot: workgroup b takes the graphs b, b + grid, ... (grid = min(G, kHeadGrid) whatever the
// device).  Per graph: x = dropout(pooled[g]) into LDS, the logits a wave per class, lse by thread 0 and dz by one thread
// per class, grad_pooled a column per thread, and the graph's share of grad_W / grad_bias / the loss sum added to the
// workgroup's own fp32 slice (plain loads and stores).  A second launch adds the slices in slice order.  No atomics: the
// same bits on every run.  The dropout rule, the logit and the row's cross entropy are tail_device.h's.
#include "tail_device.h"

using namespace sgx_tail;

namespace {

constexpr int kHeadGrid = 256;        // slices: a fixed bound, so the summation order does not depend on the device

struct HeadArgs {
    int G, P, C, grid;
    const float *pooled, *W, *bias;
    const int64_t *target;
    Dropout drop;
    uint64_t seed, step;
    const int64_t *step_dev;
    float gs;                         // grad_scale / G
    float *logits, *grad_pooled;
    float *slices;                    // [grid][C * P + C + 1]: grad_W, grad_bias, the loss sum
};

__global__ __launch_bounds__(kBlock) void head_loss_kernel(HeadArgs a)
{
#pragma clang fp contract(off)
    __shared__ float xs[kMaxP];
    __shared__ float z[kMaxC], dz[kMaxC];
    __shared__ float lse_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = a.P, C = a.C;
    const uint64_t key = dropout_key(a.seed, a.step, a.step_dev);
    const int64_t stride = (int64_t)C * P + C + 1;
    float *slice = a.slices + (int64_t)blockIdx.x * stride;
    float loss_sum = 0.0f;                                   // thread 0's
    bool first = true;
    for (int g = blockIdx.x; g < a.G; g += a.grid, first = false) {
        for (int j = tid; j < P; j += kBlock) {
            const bool keep = dropout_keep(key, (int64_t)g * P + j, a.drop.keep_from);
            xs[j] = keep ? a.pooled[(int64_t)g * P + j] * a.drop.scale : 0.0f;
        }
        __syncthreads();
        for (int c = wave; c < C; c += kBlock / 64) {
            const float s = wave_class_logit(a.W + (int64_t)c * P, xs, P, lane, a.bias, c);
            if (lane == 0) {
                z[c] = s;
                if (a.logits) a.logits[(int64_t)g * C + c] = s;
            }
        }
        __syncthreads();
        const int64_t t = a.target[g];
        const bool live = t >= 0 && t < C;
        if (tid == 0) {
            const float lse = row_cross_entropy(z, C, t).lse;
            lse_s = lse;
            if (live) loss_sum = loss_sum + (lse - z[t]);
        }
        __syncthreads();
        if (tid < C) {
            const float d = live ? (expf(z[tid] - lse_s) - (tid == t ? 1.0f : 0.0f)) * a.gs : 0.0f;
            dz[tid] = d;
            slice[(int64_t)C * P + tid] = first ? d : slice[(int64_t)C * P + tid] + d;
        }
        __syncthreads();
        for (int j = tid; j < P; j += kBlock) {
            const bool keep = dropout_keep(key, (int64_t)g * P + j, a.drop.keep_from);
            float s = 0.0f;
            for (int c = 0; c < C; ++c) s = __builtin_fmaf(dz[c], a.W[(int64_t)c * P + j], s);
            a.grad_pooled[(int64_t)g * P + j] = keep ? a.drop.scale * s : 0.0f;
        }
        for (int e = tid; e < C * P; e += kBlock) {
            const int c = e / P, j = e - c * P;
            slice[e] = first ? dz[c] * xs[j] : __builtin_fmaf(dz[c], xs[j], slice[e]);
        }
        __syncthreads();                                     // xs, z and dz are rewritten for the next graph
    }
    if (tid == 0) slice[stride - 1] = loss_sum;
}

// the slices added in slice order, an element per thread: grad_W, grad_bias, loss = sum / G
__global__ __launch_bounds__(kBlock) void head_loss_reduce_kernel(int G, int P, int C, int grid, const float *__restrict__ slices,
                                                                  float *__restrict__ grad_W, float *__restrict__ grad_bias,
                                                                  float *__restrict__ loss)
{
#pragma clang fp contract(off)
    const int64_t stride = (int64_t)C * P + C + 1;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= stride) return;
    float s = 0.0f;
    for (int b = 0; b < grid; ++b) s = s + slices[(int64_t)b * stride + e];
    if (e < (int64_t)C * P)
        grad_W[e] = s;
    else if (e < stride - 1) {
        if (grad_bias) grad_bias[e - (int64_t)C * P] = s;
    } else
        loss[0] = s / (float)G;
}

}  // namespace

extern "C" size_t sgx_head_loss_workspace_bytes(int n_graphs, int P, int C)
{
    if (!head_shape_ok(n_graphs, P, C)) return 0;
    const size_t grid = (size_t)(n_graphs < kHeadGrid ? n_graphs : kHeadGrid);
    return sgx_align_up(grid * ((size_t)C * P + C + 1) * sizeof(float), 256);
}

extern "C" int sgx_head_loss(int n_graphs, int P, int C, const float *pooled, const float *W, const float *bias,
                             const int64_t *target, float p_drop, uint64_t seed, uint64_t step, const int64_t *step_dev,
                             float grad_scale, float *loss, float *logits, float *grad_pooled, float *grad_W, float *grad_bias,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_graphs < 1 || P < 1 || C < 1) return SGX_ERR_SHAPE;
    if (!pooled || !W || !target || !loss || !grad_pooled || !grad_W || (bias && !grad_bias)) return SGX_ERR_NULL;
    if (!(p_drop >= 0.0f && p_drop < 1.0f) || P > kMaxP || C > kMaxC) return SGX_ERR_UNSUPPORTED;
    const size_t need = sgx_head_loss_workspace_bytes(n_graphs, P, C);
    if (!workspace || workspace_bytes < need) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256) return SGX_ERR_ALIGN;
    HeadArgs a;
    a.G = n_graphs, a.P = P, a.C = C, a.grid = n_graphs < kHeadGrid ? n_graphs : kHeadGrid;
    a.pooled = pooled, a.W = W, a.bias = bias, a.target = target;
    a.drop = dropout_of(p_drop);
    a.seed = seed, a.step = step, a.step_dev = step_dev;
    a.gs = grad_scale / (float)n_graphs;
    a.logits = logits, a.grad_pooled = grad_pooled;
    a.slices = (float *)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(head_loss_kernel, dim3(a.grid), dim3(kBlock), 0, s, a);
    SGX_LAUNCH_CHECK();
    const int64_t stride = (int64_t)C * P + C + 1;
    hipLaunchKernelGGL(head_loss_reduce_kernel, dim3((unsigned)((stride + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, n_graphs, P, C,
                       a.grid, (const float *)workspace, grad_W, bias ? grad_bias : nullptr, loss);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
