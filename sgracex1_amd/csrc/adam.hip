// Multi-tensor Adam in one launch (sgx_adam_step, include/sgx.h "the optimiser"): torch.optim.Adam without amsgrad on up
// to SGX_ADAM_MAX_TENSORS fp32 tensors, the tensor table passed by value in the kernel arguments (nothing is uploaded),
// driven by a step counter that lives on the device -- so one captured call is the right update at every replay.
// Optionally each updated parameter is also written transposed in the layer kernels' element type (the W^T a stack
// forward takes), which saves the per-step transpose(...).to(dtype).contiguous().
//
// Element-wise: a workgroup takes kChunk consecutive elements of one tensor; nothing is summed across elements, so the
// grid has no part in the result.  A trailing one-thread launch leaves t in the counter.
#include "sgx_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 1024;          // elements per workgroup

struct AdamTable {
    sgx_adam_tensor t[SGX_ADAM_MAX_TENSORS];
    int32_t first[SGX_ADAM_MAX_TENSORS + 1];      // the first workgroup of every tensor
    int32_t n;
    float lr, b1, ob1, b2, ob2, eps, wd;          // (float)lr, (float)beta1, (float)(1 - beta1), ... rounded on the host
    double beta1, beta2;
    const int64_t *step;
};

template <typename T>
__device__ __forceinline__ void store_t(void *out, int64_t i, int rows, int cols, float p)
{
    const int64_t r = i / cols, c = i - r * cols;
    ((T *)out)[c * rows + r] = (T)p;
}

__global__ __launch_bounds__(kBlock) void adam_kernel(AdamTable a)
{
#pragma clang fp contract(off)
    __shared__ float corr[2];                     // step_size = lr / bc1, sqrt(bc2)
    if (threadIdx.x == 0) {
        const double t = (double)(a.step[0] + 1);
        const float bc1 = (float)(1.0 - pow(a.beta1, t));
        corr[0] = a.lr / bc1;
        corr[1] = (float)sqrt(1.0 - pow(a.beta2, t));
    }
    __syncthreads();
    const float step_size = corr[0], sqrt_bc2 = corr[1];
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.first[k + 1]) ++k;
    const sgx_adam_tensor T = a.t[k];
    const int64_t base = (int64_t)((int)blockIdx.x - a.first[k]) * kChunk;
    for (int64_t i = base + threadIdx.x; i < base + kChunk && i < T.n; i += kBlock) {
        float p = T.param[i], g = T.grad[i], m = T.m[i], v = T.v[i];
        if (a.wd != 0.0f) {
            const float r = a.wd * p;
            g = g + r;
        }
        const float r1 = a.b1 * m, r2 = a.ob1 * g;
        m = r1 + r2;
        const float r3 = a.b2 * v, r4 = g * g;
        const float r5 = a.ob2 * r4;
        v = r3 + r5;
        const float s = sqrtf(v) / sqrt_bc2;
        const float denom = s + a.eps;
        const float q = m / denom;
        const float u = step_size * q;
        p = p - u;
        T.param[i] = p, T.m[i] = m, T.v[i] = v;
        if (T.param_t_out) {
            if (T.dtype_t == SGX_F16)
                store_t<f16>(T.param_t_out, i, T.rows, T.cols, p);
            else
                store_t<float>(T.param_t_out, i, T.rows, T.cols, p);
        }
    }
}

__global__ void adam_advance_kernel(int64_t *step)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) step[0] = step[0] + 1;
}

}  // namespace

extern "C" int sgx_adam_step(const sgx_adam_desc *d, void *stream)
{
    if (!d || !d->step) return SGX_ERR_NULL;
    if (d->n_tensors < 0 || d->n_tensors > SGX_ADAM_MAX_TENSORS) return SGX_ERR_SHAPE;
    if (!(d->lr >= 0.0) || !(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0) || !(d->eps >= 0.0) ||
        !(d->weight_decay >= 0.0))
        return SGX_ERR_UNSUPPORTED;
    AdamTable a = {};
    int64_t blocks = 0;
    for (int k = 0; k < d->n_tensors; ++k) {
        const sgx_adam_tensor &t = d->tensor[k];
        if (t.n < 0) return SGX_ERR_SHAPE;
        if (t.n == 0 || !t.grad) continue;                          // as torch skips p.grad is None
        if (!t.param || !t.m || !t.v) return SGX_ERR_NULL;
        if (t.param_t_out) {
            if (t.rows < 1 || t.cols < 1 || (int64_t)t.rows * t.cols != t.n) return SGX_ERR_SHAPE;
            if (t.dtype_t != SGX_F16 && t.dtype_t != SGX_F32) return SGX_ERR_UNSUPPORTED;
        }
        a.first[a.n] = (int32_t)blocks;
        a.t[a.n++] = t;
        blocks += (t.n + kChunk - 1) / kChunk;
        if (blocks > 0x7fffffff) return SGX_ERR_UNSUPPORTED;
    }
    a.first[a.n] = (int32_t)blocks;
    a.lr = (float)d->lr, a.eps = (float)d->eps, a.wd = (float)d->weight_decay;
    a.b1 = (float)d->beta1, a.ob1 = (float)(1.0 - d->beta1), a.b2 = (float)d->beta2, a.ob2 = (float)(1.0 - d->beta2);
    a.beta1 = d->beta1, a.beta2 = d->beta2;
    a.step = d->step;
    hipStream_t s = (hipStream_t)stream;
    if (blocks > 0) {
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
        SGX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, s, d->step);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
