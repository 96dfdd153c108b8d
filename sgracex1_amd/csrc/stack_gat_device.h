// The GAT stage of the small-graph stack and the one kernel around it, shared by stack_gat.hip (sgx_gat_stack_forward)
// and stack_quant.hip (sgx_quant_stack_forward, the same launch with a layer's quantiser in the stages).
#pragma once
#include "stack_device.h"
#include "gat_device.h"

namespace {

struct GatStackArgs {
    StackArgs s;
    int gat[kMaxLayers];
    const void *att[kMaxLayers];
    float alpha[kMaxLayers];
};

constexpr int kScoreLanes = 8;                                   // lanes per row of steps 1 and 2
constexpr float kLog2e = 1.44269504088896340736f;

// bytes of the four score / softmax arrays behind the tiles
size_t score_bytes(int rows) { return (size_t)4 * rows * sizeof(float); }

// x_e of a stored entry of row i (score si), or -inf when it is masked or leaves the group: such an entry reads nothing
// (with a quantiser the mask is on the quantised value)
template <typename T, typename Q>
__device__ __forceinline__ float entry_score(const GatStackArgs &g, const Q &q, int l, int e, int r0, int nr, float si,
                                             const float *__restrict__ s2, float alpha, int *c_out)
{
    const int c = g.s.col[e] - r0;
    *c_out = c;
    if ((unsigned)c >= (unsigned)nr) return -INFINITY;               // (the plan admits no such edge)
    if (!(stack_q_adj(q, l, Elem<T>::to_f32(static_cast<const T *>(g.s.val)[e])) > 0.0f)) return -INFINITY;
    return leaky(si + s2[c], alpha);
}

// XD = D_l = act(softmax-weighted sum of the rows of Hs), also to the caller's D; sc: the four [rows] arrays.  With a
// quantiser: the attention vector on the weights' grid as it is read, D = act(sum) * deq_factor, the X tile through
// stack_next_x.
template <typename T, typename Q = StackPlain>
__device__ __forceinline__ void stack_gat_aggregate(const GatStackArgs &g, int l, int r0, int nr, T *__restrict__ XD,
                                                    const T *__restrict__ Hs, float *__restrict__ sc, const Q &q = Q())
{
    const StackArgs &a = g.s;
    const int P = a.P[l], pitch = a.pitch;
    float *const s1 = sc, *const s2 = sc + a.rows, *const rm = sc + 2 * a.rows, *const ri = sc + 3 * a.rows;
    const float alpha = g.alpha[l];
    const int t8 = threadIdx.x & (kScoreLanes - 1), row8 = threadIdx.x / kScoreLanes;

    // 1. the two scores of every row of the group
    {
        const T *__restrict__ att = static_cast<const T *>(g.att[l]);
        for (int i = row8; i < nr; i += kBlock / kScoreLanes) {
            const T *h = Hs + (size_t)i * pitch;
            float p1 = 0.0f, p2 = 0.0f;
            for (int j = t8; j < P; j += kScoreLanes) {
                const float hv = Elem<T>::to_f32(h[j]);
                p1 = __builtin_fmaf(hv, stack_q_w(q, l, Elem<T>::to_f32(att[j])), p1);
                p2 = __builtin_fmaf(hv, stack_q_w(q, l, Elem<T>::to_f32(att[P + j])), p2);
            }
#pragma unroll
            for (int off = kScoreLanes / 2; off > 0; off >>= 1) {
                p1 += __shfl_xor(p1, off, kScoreLanes);
                p2 += __shfl_xor(p2, off, kScoreLanes);
            }
            if (t8 == 0) {
                s1[i] = p1;
                s2[i] = p2;
            }
        }
    }
    __syncthreads();

    // 2. the row statistics: m_i over the live entries, then 1 / sum exp(x - m_i); a row without a live entry keeps 0, 0
    for (int i = row8; i < nr; i += kBlock / kScoreLanes) {
        const int e0 = a.rowptr[r0 + i], e1 = a.rowptr[r0 + i + 1];
        const float si = s1[i];
        int c;
        float m = -INFINITY;
        for (int e = e0 + t8; e < e1; e += kScoreLanes) m = fmaxf(m, entry_score<T>(g, q, l, e, r0, nr, si, s2, alpha, &c));
#pragma unroll
        for (int off = kScoreLanes / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kScoreLanes));
        float sum = 0.0f;
        if (m != -INFINITY) {                                          // (the same for the row's eight lanes)
            for (int e = e0 + t8; e < e1; e += kScoreLanes) {
                const float x = entry_score<T>(g, q, l, e, r0, nr, si, s2, alpha, &c);
                if (x != -INFINITY) sum += __builtin_amdgcn_exp2f((x - m) * kLog2e);
            }
        }
#pragma unroll
        for (int off = kScoreLanes / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kScoreLanes);
        if (t8 == 0) {
            rm[i] = m != -INFINITY ? m : 0.0f;
            ri[i] = sum > 0.0f ? 1.0f / sum : 0.0f;
        }
    }
    __syncthreads();

    // 3. the aggregate: `lpr` lanes per row (a power of two, one lane per four columns), the weights of lpr entries at a
    //    time formed one per lane and read round the group
    {
        const int nch = (P + 3) / 4;
        int lpr = 1;
        while (lpr < nch) lpr <<= 1;                                    // <= 64: P <= 256
        const int t = threadIdx.x & (lpr - 1), c0 = 4 * t;
        T *__restrict__ Dg = static_cast<T *>(a.D[l]);
        const int64_t ldd = a.ldd[l];
        const int relu = a.relu[l];
        const sgx_epilogue ep = stack_ep_d(q, l);
        for (int i = threadIdx.x / lpr; i < nr; i += kBlock / lpr) {
            const int e0 = a.rowptr[r0 + i], e1 = a.rowptr[r0 + i + 1];
            const float si = s1[i], m = rm[i], inv = ri[i];
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int base = e0; base < e1; base += lpr) {
                int c = -1;
                float w = 0.0f;
                if (base + t < e1) {
                    const float x = entry_score<T>(g, q, l, base + t, r0, nr, si, s2, alpha, &c);
                    if (x != -INFINITY) w = __builtin_amdgcn_exp2f((x - m) * kLog2e) * inv;
                    else c = -1;
                }
                const int n = e1 - base < lpr ? e1 - base : lpr;
                for (int j = 0; j < n; ++j) {
                    const int cj = __shfl(c, j, lpr);
                    const float wj = __shfl(w, j, lpr);
                    if (cj < 0 || c0 >= P) continue;
                    const T *h = Hs + (size_t)cj * pitch + c0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(wj, Elem<T>::to_f32(h[u]), acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u >= P) break;
                const T v = finish_value<T>(acc[u], relu, ep);
                XD[(size_t)i * pitch + c0 + u] = stack_next_x<T>(q, l, a.n_layers, v);
                if (Dg) Dg[(int64_t)(r0 + i) * ldd + c0 + u] = v;
            }
        }
    }
}

// the kernel's body: every layer, then the readout, for the workgroup's group of graphs
template <typename T, typename Q>
__device__ __forceinline__ void gat_stack_body(const GatStackArgs &g, const Q &q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stack_lds[];
    const StackArgs &a = g.s;
    T *const XD = reinterpret_cast<T *>(stack_lds);                 // X_l, then D_l      [rows][pitch]
    T *const Hs = XD + (size_t)a.rows * a.pitch;                    // H_l                [rows][pitch]
    float *const sc = reinterpret_cast<float *>(Hs + (size_t)a.rows * a.pitch);   // s1, s2, m, 1/l  [4][rows]
    const StackGroup grp = stack_group(a.group_graph, a.graph_ptr, a.rows, blockIdx.x);
    if (grp.gf >= grp.gl) return;
    const int r0 = grp.r0, nr = grp.nr;

    for (int l = 0; l < a.n_layers; ++l) {
        stack_form_h<T, Q>(a, l, r0, nr, XD, Hs, q);
        __syncthreads();
        if (g.gat[l]) stack_gat_aggregate<T, Q>(g, l, r0, nr, XD, Hs, sc, q);
        else stack_gcn_aggregate<T, Q>(a, l, r0, nr, XD, Hs, q);
        __syncthreads();
    }
    stack_readout<T>(a, grp.gf, grp.gl, r0, XD);
}

// two workgroups per CU: 2 x (64 KiB of tiles + the score arrays) of the CU's 160 KiB, 8 of its 32 wavefronts
template <typename T>
__global__ __launch_bounds__(kBlock, 2) void gat_stack_kernel(GatStackArgs g)
{
    gat_stack_body<T>(g, StackPlain());
}

// the same launch with the layers' quantisers (instantiated for fp32 only, in stack_quant.hip)
template <typename T>
__global__ __launch_bounds__(kBlock, 2) void quant_stack_kernel(GatStackArgs g, StackQuant q)
{
    gat_stack_body<T>(g, q);
}

// the launch; kernel: gat_stack_kernel<T> or quant_stack_kernel, optin: that kernel's, extra: what follows GatStackArgs in
// its arguments
template <typename Kernel, typename... Extra>
int launch_stack_kernel(Kernel kernel, sgx_lds_optin &optin, const GatStackArgs &g, int n_groups, size_t lds, hipStream_t s,
                        const Extra &...extra)
{
    if (lds > (size_t)kStackLds) {
        // tiles that fill 64 KiB (fp32 at width 252: 32 rows of 2 KiB) plus the score arrays
        const int rc = sgx_raise_dynamic_lds(kernel, optin, kStackLds + score_bytes(SGX_STACK_ROWS_CAP));
        if (rc != SGX_OK) return rc;
    }
    hipLaunchKernelGGL(kernel, dim3(n_groups), dim3(kBlock), lds, s, g, extra...);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

// the kernel's arguments and its LDS bytes from a descriptor whose layers carry gat_mode / attention / alpha
template <typename Desc>
GatStackArgs gat_stack_args(const Desc *d, size_t *lds)
{
    const sgx_batch_plan *p = d->plan;
    GatStackArgs g;
    g.s = stack_args(d);
    bool any = false;
    for (int l = 0; l < kMaxLayers; ++l) {
        const bool gat = l < d->n_layers && d->layer[l].gat_mode == 1;
        any = any || gat;
        g.gat[l] = gat ? 1 : 0;
        g.att[l] = gat ? d->layer[l].attention : nullptr;
        g.alpha[l] = gat ? d->layer[l].alpha : 0.0f;
    }
    *lds = (size_t)2 * p->rows * g.s.pitch * sgx_elem_size(d->dtype) + (any ? score_bytes(p->rows) : 0);
    return g;
}

// what a layer with gat_mode / attention adds to check_stack_desc
template <typename Layer>
int check_gat_layer(const Layer &L)
{
    if (L.gat_mode != 0 && L.gat_mode != 1) return (int)SGX_ERR_UNSUPPORTED;
    if (L.gat_mode == 1 && !L.attention) return (int)SGX_ERR_NULL;
    return (int)SGX_OK;
}

}  // namespace
