// The small-graph stack's backward (sgx_stack_backward): the weight gradients of the stack sgx_stack_forward (stack.hip) ran,
// on the same plan groups.  A persistent grid: workgroup w walks the groups w, w + grid, ... and runs, per group, the
// layers from the top down with g_l, G_l (fp32) and X_l (dtype) in LDS.  Its weight gradients go to its own slice of the
// workspace; a second launch adds the slices in order.
#include "stack_device.h"

namespace {

constexpr int kGradGrid = 512;        // two 64 KiB workgroups per CU of an MI355X; fixed, so the slicing (and the bits)
                                      // do not depend on the device
constexpr int kSparseRegK = 16;       // a sparse layer 0 this narrow keeps its weight gradient in registers

struct GradArgs {
    int n_layers, gemm0, pitch_t, pitch_f, rows, n_groups, slice;
    int relu[kMaxLayers], K[kMaxLayers], P[kMaxLayers], off[kMaxLayers];
    const float *W[kMaxLayers];
    const void *D[kMaxLayers];
    int64_t ldd[kMaxLayers];
    float *G[kMaxLayers];
    const int32_t *graph_ptr, *group_graph;
    const int32_t *rowptr, *col;
    const void *val;
    const int32_t *rowptr_f, *col_f;
    const void *val_f;
    const float *grad_pooled;
    float *ws;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void gcn_stack_backward_kernel(GradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stack_lds[];
    float *const Gs = reinterpret_cast<float *>(stack_lds);                // G_l = A . g_l   [rows][pitch_f]
    float *const gs = Gs + (size_t)a.rows * a.pitch_f;                      // g_l              [rows][pitch_f]
    T *const XD = reinterpret_cast<T *>(gs + (size_t)a.rows * a.pitch_f);   // X_l = D_{l-1}    [rows][pitch_t]
    const int pf = a.pitch_f, pt = a.pitch_t;
    const int L = a.n_layers;
    const T *__restrict__ val = static_cast<const T *>(a.val);
    float *const slice = a.ws + (size_t)blockIdx.x * a.slice;
    // sparse layer 0 of at most kSparseRegK columns: thread p keeps dW_0[0..K-1][p] in registers over all its groups
    const bool sparse_reg = a.gemm0 == 0 && a.K[0] <= kSparseRegK;
    float dw0[kSparseRegK];
#pragma unroll
    for (int k = 0; k < kSparseRegK; ++k) dw0[k] = 0.0f;

    const int n_iter = a.n_groups > 0 ? a.n_groups : 1;        // (an empty batch: one empty group, zero slices)
    for (int grp = blockIdx.x; grp < n_iter; grp += gridDim.x) {
        const bool first = grp == (int)blockIdx.x;             // the workgroup's first group writes its slice
        const StackGroup sg = grp < a.n_groups ? stack_group(a.group_graph, a.graph_ptr, a.rows, grp) : StackGroup{0, 0, 0, 0};
        const int gf = sg.gf, gl = sg.gl, r0 = sg.r0, nr = sg.nr;

        // g_{L-1}: each row its graph's pooled gradient over the graph's size, rounded to dtype, masked by D_{L-1}
        {
            const int P = a.P[L - 1];
            const T *__restrict__ Dg = static_cast<const T *>(a.D[L - 1]);
            const int64_t ldd = a.ldd[L - 1];
            const int relu = a.relu[L - 1];
            const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
            for (int g = gf + wave; g < gl; g += kBlock / 64) {
                const int s0 = a.graph_ptr[g] - r0, s1 = a.graph_ptr[g + 1] - r0;
                if (s1 <= s0) continue;
                const float inv = 1.0f / (float)(s1 - s0);
                for (int j = lane; j < P; j += 64) {
                    const float v = Elem<T>::to_f32(Elem<T>::from_f32(a.grad_pooled[(int64_t)g * P + j] * inv));
                    for (int r = s0; r < s1; ++r) {
                        const bool dead = relu && Elem<T>::to_f32(Dg[(int64_t)(r0 + r) * ldd + j]) == 0.0f;
                        gs[(size_t)r * pf + j] = dead ? 0.0f : v;
                    }
                }
            }
        }
        __syncthreads();

        for (int l = L - 1; l >= 0; --l) {
            const int K = a.K[l], P = a.P[l];
            const int nch = (P + 3) / 4;
            // G = A . g: rows of A from global, columns rebased to the group's first row, g gathered from LDS
            float *__restrict__ Gout = a.G[l];
            for (int it = threadIdx.x; it < nr * nch; it += kBlock) {
                const int i = it / nch, c0 = (it - i * nch) * 4;
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                const int e0 = a.rowptr[r0 + i], e1 = a.rowptr[r0 + i + 1];
                for (int e = e0; e < e1; ++e) {
                    const int c = a.col[e] - r0;
                    if ((unsigned)c >= (unsigned)nr) continue;         // (the plan admits no such edge)
                    const float w = Elem<T>::to_f32(val[e]);
                    const f32x4 h = *reinterpret_cast<const f32x4 *>(gs + (size_t)c * pf + c0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(w, h[u], acc[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (c0 + u >= P) break;
                    Gs[(size_t)i * pf + c0 + u] = acc[u];
                    if (Gout) Gout[(int64_t)(r0 + i) * P + c0 + u] = acc[u];
                }
            }
            // X_l into LDS (D_l, which it replaces, has already masked g_l); a CSR layer 0 puts the group's feature
            // entries there instead (rebased row offsets, columns, fp32 values) when they fit, so that the serial
            // per-column walk below reads LDS rather than waiting on global loads row after row
            const T *__restrict__ vf = static_cast<const T *>(a.val_f);
            int32_t *const lrow = reinterpret_cast<int32_t *>(XD);
            int32_t *const lcol = lrow + ((nr + 1 + 3) & ~3);
            float *lx = nullptr;
            bool staged = false;                                       // (uniform across the workgroup)
            if (l == 0 && a.gemm0 == 0 && nr > 0) {
                const int e_base = a.rowptr_f[r0];
                const int n_e = a.rowptr_f[r0 + nr] - e_base;
                lx = reinterpret_cast<float *>(lcol + ((n_e + 3) & ~3));
                staged = ((size_t)((nr + 1 + 3) & ~3) + 2 * (size_t)((n_e + 3) & ~3)) * sizeof(int32_t) <=
                         (size_t)a.rows * pt * sizeof(T);
                if (staged) {
                    for (int i = threadIdx.x; i <= nr; i += kBlock) lrow[i] = a.rowptr_f[r0 + i] - e_base;
                    for (int e = threadIdx.x; e < n_e; e += kBlock) {
                        lcol[e] = a.col_f[e_base + e];
                        lx[e] = Elem<T>::to_f32(vf[e_base + e]);
                    }
                }
            }
            if (l > 0 || a.gemm0 == 1) {
                const T *__restrict__ X = static_cast<const T *>(l > 0 ? a.D[l - 1] : a.val_f);
                const int64_t ldx = l > 0 ? a.ldd[l - 1] : K;
                for (int it = threadIdx.x; it < nr * K; it += kBlock) {
                    const int i = it / K, k = it - i * K;
                    XD[(size_t)i * pt + k] = X[(int64_t)(r0 + i) * ldx + k];
                }
            }
            __syncthreads();

            // dW_l += X_l^T . G_l over the group's rows in order
            float *__restrict__ dw = slice + a.off[l];
            if (l == 0 && a.gemm0 == 0) {
                // sparse X: thread p owns column p and walks the rows and their entries in order
                const int p = threadIdx.x;
                if (p < P) {
                    if (!sparse_reg && first)
                        for (int k = 0; k < K; ++k) dw[(size_t)k * P + p] = 0.0f;
                    for (int i = 0; i < nr; ++i) {
                        const float gv = Gs[(size_t)i * pf + p];
                        const int e0 = staged ? lrow[i] : a.rowptr_f[r0 + i];
                        const int e1 = staged ? lrow[i + 1] : a.rowptr_f[r0 + i + 1];
                        for (int e = e0; e < e1; ++e) {
                            const int k = staged ? lcol[e] : a.col_f[e];
                            if ((unsigned)k >= (unsigned)K) continue;      // (the chain's X^T has no such entry)
                            const float x = staged ? lx[e] : Elem<T>::to_f32(vf[e]);
                            if (sparse_reg) {
#pragma unroll
                                for (int kk = 0; kk < kSparseRegK; ++kk)
                                    if (kk == k) dw0[kk] = __builtin_fmaf(x, gv, dw0[kk]);
                            } else {
                                float *w = dw + (size_t)k * P + p;
                                *w = __builtin_fmaf(x, gv, *w);
                            }
                        }
                    }
                }
            } else {
                // dense X: a thread owns (k, four consecutive p) items of the slice
                const int nq = (P + 3) / 4;
                for (int it = threadIdx.x; it < K * nq; it += kBlock) {
                    const int k = it / nq, p0 = (it - k * nq) * 4;
                    float acc[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = (first || p0 + u >= P) ? 0.0f : dw[(size_t)k * P + p0 + u];
                    for (int i = 0; i < nr; ++i) {
                        const float x = Elem<T>::to_f32(XD[(size_t)i * pt + k]);
                        const f32x4 gv = *reinterpret_cast<const f32x4 *>(Gs + (size_t)i * pf + p0);
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(x, gv[u], acc[u]);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (p0 + u < P) dw[(size_t)k * P + p0 + u] = acc[u];
                }
            }

            // g_{l-1} = dtype(G_l . W_l^T) on the matrix cores (sgx_xw_dense's fp32 layout), masked by D_{l-1} = X_l
            if (l > 0) {
                const int relu = a.relu[l - 1];
                xw_dense_lds_apply<float>(Gs, pf, nr, P, K, a.W[l], [&](int m, int n, float v) {
                    const float r = Elem<T>::to_f32(Elem<T>::from_f32(v));
                    const bool dead = relu && Elem<T>::to_f32(XD[(size_t)m * pt + n]) == 0.0f;
                    gs[(size_t)m * pf + n] = dead ? 0.0f : r;
                });
            }
            __syncthreads();
        }
    }
    if (sparse_reg && (int)threadIdx.x < a.P[0]) {
        float *__restrict__ dw = slice + a.off[0];
        for (int k = 0; k < a.K[0]; ++k) {
            float v = 0.0f;
#pragma unroll
            for (int kk = 0; kk < kSparseRegK; ++kk)
                if (kk == k) v = dw0[kk];
            dw[(size_t)k * a.P[0] + threadIdx.x] = v;
        }
    }
}

struct GradOut {
    int off[kMaxLayers + 1], size[kMaxLayers];
    float *grad_W[kMaxLayers];
};

// grad_W = the slices added in slice order (the first added to 0)
__global__ __launch_bounds__(kBlock) void stack_grad_reduce_kernel(int n_slices, int slice, const float *__restrict__ ws,
                                                                   GradOut o)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= o.off[kMaxLayers]) return;
    float s = 0.0f;
    int w = 0;
    for (; w + 16 <= n_slices; w += 16) {              // sixteen loads in flight, added in slice order
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = ws[(size_t)(w + j) * slice + idx];
#pragma unroll
        for (int j = 0; j < 16; ++j) s += v[j];
    }
    for (; w < n_slices; ++w) s += ws[(size_t)w * slice + idx];
    int l = 0;
    while (l + 1 < kMaxLayers && idx >= o.off[l + 1]) ++l;
    if (idx - o.off[l] < o.size[l]) o.grad_W[l][idx - o.off[l]] = s;       // (not the padding after a block)
}

int check_grad(const sgx_stack_grad_desc *d)
{
    int rc = stack_check_head(d);
    if (rc != SGX_OK) return rc;
    for (int l = 0; l < d->n_layers; ++l) {
        const sgx_stack_grad_layer &L = d->layer[l];
        if ((rc = stack_check_layer_shape(d, l)) != SGX_OK) return rc;
        if (!L.W || !L.grad_W) return SGX_ERR_NULL;
        if ((l < d->n_layers - 1 || L.relu) && !L.D && d->n_rows > 0) return SGX_ERR_NULL;
    }
    if (d->n_graphs > 0 && !d->grad_pooled) return SGX_ERR_NULL;
    return stack_check_batch(d);
}

// what the fused backward takes: a backward plan that fits, widths within it
int grad_supported(const sgx_stack_grad_desc *d)
{
    const sgx_batch_plan *p = d->plan;
    if (p->kind != SGX_BATCH_BACKWARD || p->dtype != d->dtype || !p->fits || p->rows < 1 || p->max_width > kStackMaxWidth)
        return SGX_ERR_UNSUPPORTED;
    if (p->n_rows > 0 && p->n_groups < 1) return SGX_ERR_UNSUPPORTED;
    return stack_widths_fit(d) ? SGX_OK : SGX_ERR_UNSUPPORTED;
}

int grad_grid(const sgx_batch_plan *p) { return p->n_groups < 1 ? 1 : (p->n_groups < kGradGrid ? p->n_groups : kGradGrid); }

// floats per slice, each layer's block starting on 16 bytes
size_t grad_slice(const sgx_stack_grad_desc *d, int *off)
{
    size_t n = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        if (off) off[l] = (int)n;
        n += ((size_t)d->layer[l].M_fea * d->layer[l].P_w + 3) / 4 * 4;
    }
    return n;
}

size_t grad_workspace(const sgx_stack_grad_desc *d)
{
    return sgx_align_up((size_t)grad_grid(d->plan) * grad_slice(d, nullptr) * sizeof(float), 256);
}

int run_backward(const sgx_stack_grad_desc *d, hipStream_t s)
{
    const sgx_batch_plan *p = d->plan;
    GradArgs a;
    a.n_layers = d->n_layers;
    a.gemm0 = d->layer[0].gemm_mode;
    a.pitch_t = lds_pitch(d->dtype, p->max_width);
    a.pitch_f = lds_pitch(SGX_F32, p->max_width);
    a.rows = p->rows;
    a.n_groups = p->n_groups;
    GradOut o;
    a.slice = (int)grad_slice(d, a.off);
    for (int l = 0; l < kMaxLayers; ++l) {
        const bool live = l < d->n_layers;
        const sgx_stack_grad_layer &L = d->layer[live ? l : 0];
        a.relu[l] = live ? (L.relu ? 1 : 0) : 0;
        a.K[l] = live ? L.M_fea : 0;
        a.P[l] = live ? L.P_w : 0;
        if (!live) a.off[l] = a.slice;
        a.W[l] = live ? L.W : nullptr;
        a.D[l] = live ? L.D : nullptr;
        a.ldd[l] = live ? layer_ldd(L) : 0;
        a.G[l] = live ? L.G : nullptr;
        o.off[l] = live ? a.off[l] : a.slice;
        o.grad_W[l] = live ? L.grad_W : nullptr;
        o.size[l] = live ? L.M_fea * L.P_w : 0;
    }
    // the reduction reads layer l's block [off[l], off[l] + M P); the padding between blocks maps to no layer
    o.off[kMaxLayers] = a.off[d->n_layers - 1] + d->layer[d->n_layers - 1].M_fea * d->layer[d->n_layers - 1].P_w;
    a.graph_ptr = d->graph_ptr;
    a.group_graph = p->group_graph;
    a.rowptr = d->rowPtr_adj;
    a.col = d->columnIndex_adj;
    a.val = d->values_adj;
    a.rowptr_f = d->rowPtr_fea;
    a.col_f = d->columnIndex_fea;
    a.val_f = d->values_fea;
    a.grad_pooled = d->grad_pooled;
    a.ws = static_cast<float *>(d->workspace);
    const int grid = grad_grid(p);
    const size_t lds = (size_t)p->rows * grad_row_bytes(d->dtype, p->max_width);
    if (d->dtype == SGX_F16)
        hipLaunchKernelGGL(gcn_stack_backward_kernel<f16>, dim3(grid), dim3(kBlock), lds, s, a);
    else
        hipLaunchKernelGGL(gcn_stack_backward_kernel<float>, dim3(grid), dim3(kBlock), lds, s, a);
    SGX_LAUNCH_CHECK();
    hipLaunchKernelGGL(stack_grad_reduce_kernel, dim3((unsigned)((o.off[kMaxLayers] + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       grid, a.slice, a.ws, o);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

}  // namespace

extern "C" size_t sgx_stack_backward_workspace_bytes(const sgx_stack_grad_desc *d)
{
    if (check_grad(d) != SGX_OK || grad_supported(d) != SGX_OK) return 0;
    return grad_workspace(d);
}

extern "C" int sgx_stack_backward(const sgx_stack_grad_desc *d, void *stream)
{
    int rc = check_grad(d);
    if (rc != SGX_OK) return rc;
    rc = grad_supported(d);
    if (rc != SGX_OK) return rc;
    if (!d->workspace || d->workspace_bytes < grad_workspace(d)) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)d->workspace % 256 != 0) return SGX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (d->n_rows == 0) {
        // no rows: every weight gradient is 0 (and there is no G to write)
        for (int l = 0; l < d->n_layers; ++l)
            SGX_HIP_CHECK(hipMemsetAsync(d->layer[l].grad_W, 0, sizeof(float) * (size_t)d->layer[l].M_fea * d->layer[l].P_w, s));
        return SGX_OK;
    }
    return run_backward(d, s);
}
