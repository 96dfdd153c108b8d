// The small-graph stack's backward with GAT layers, shared by stack_gat_bwd.hip (sgx_gat_stack_backward) and
// stack_quant_bwd.hip (sgx_quant_stack_backward, the same launch with a layer's quantiser in the forward quantities it
// forms again): sgx_stack_backward (stack_bwd.hip) with a per-layer choice of P in G_l = P . g_l -- the adjacency
// (gat_mode 0, that kernel's arithmetic) or the edge softmax S (gat_mode 1), formed again from X_l and the parameters --
// and, for a GAT layer, the gradient of its attention vector.  The same SGX_BATCH_BACKWARD plans, the same persistent
// grid, slices and reduction; a fourth fp32 tile (Wh) and six floats per row (s1, s2, m, 1 / l, rs, g1) behind
// sgx_stack_backward's three tiles.
// The GCN steps are restated here and not shared with stack_bwd.hip, so that sgx_stack_backward's kernel keeps its code.
//
// The policy Q is stack_device.h's: StackPlain compiles every hook out; StackQuantGrad (StackQuant plus the stored
// quantised adjacency) puts a quantised GAT layer's S and E on the quantised forward's operands -- H_q = requant(X_q . W_q),
// the attention vector on the weights' grid, the mask on the quantised adjacency value -- and then forms Wh a second time
// from the unquantised operands over the same tile, so that everything a gradient multiplies with is unquantised
// (FPYNQ_GAT.backward).  GCN layers never see the quantiser.
#pragma once
#include "stack_device.h"
#include "gat_device.h"

namespace {

constexpr int kGatGradGrid = 512;         // sgx_stack_backward's: fixed, so the slicing (and the bits) do not depend on the device
constexpr int kGatSparseRegK = 16;        // a sparse layer 0 this narrow keeps its weight gradient in registers
constexpr int kGatScoreLanes = 8;         // lanes per row of the score and statistics steps
constexpr float kGatLog2e = 1.44269504088896340736f;
constexpr size_t kGatLdsLimit = 160 * 1024;   // what a workgroup on gfx950 may declare
constexpr int kGatRowFloats = 6;          // s1, s2, m, 1 / l, rs, g1

struct GatGradArgs {
    int n_layers, gemm0, pitch_t, pitch_f, rows, n_groups, slice;
    int relu[kMaxLayers], K[kMaxLayers], P[kMaxLayers], off[kMaxLayers];
    int gat[kMaxLayers], aoff[kMaxLayers];        // aoff: the layer's grad_attention block in a slice
    float alpha[kMaxLayers];
    const float *W[kMaxLayers], *att[kMaxLayers];
    const void *D[kMaxLayers];
    int64_t ldd[kMaxLayers];
    float *G[kMaxLayers], *S[kMaxLayers], *E[kMaxLayers];
    const int32_t *graph_ptr, *group_graph;
    const int32_t *rowptr, *col;
    const void *val;
    const int32_t *rowptr_f, *col_f;
    const void *val_f;
    const float *grad_pooled;
    float *ws;
};

// StackQuant for the backward: values_adj_q, the adjacency as a layer with SGX_QUANT_ADJ_DONE masks with it
struct StackQuantGrad : StackQuant {
    const float *val_q;
};

// the layer forms its S and E under a quantiser
template <typename Q> __device__ __forceinline__ bool stack_q_on(const Q &q, int l)
{
    if constexpr (Q::kQuant) return q.on[l] != 0;
    return false;
}

// a group's CSR feature entries in LDS (rebased row offsets, columns, fp32 values), or the arrays in global memory
struct FeaRows {
    bool staged;
    const int32_t *lrow, *lcol;
    const float *lx;
};

// Wh[0:nr][0:P] = fp32(X[0:nr][0:K]) . W, X (dtype) in LDS, W [K][P] fp32 in global: xw_dense_lds_apply's items, MFMA
// layout and K order (sgx_xw_dense's fp32 kernel), the operands fetched element by element.  With layer l's quantiser:
// X and W on their grids as they are fetched (pad elements stay 0) and the re-quantisation on the store, as
// xw_dense_lds forms H in the forward.
template <typename T, typename Q>
__device__ __forceinline__ void wh_dense_lds(const T *__restrict__ X, int pt, int nr, int K, int P, const float *__restrict__ W,
                                             float *__restrict__ Wh, int pf, const Q &q, int l)
{
    const bool qon = stack_q_on(q, l);
    const sgx_epilogue ep = stack_ep_h(q, l);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int l15 = lane & 15, lq = lane >> 4;
    const int n_rt = (nr + 15) / 16, n_cg = (P + 63) / 64;
    for (int item = wave; item < n_rt * n_cg; item += kBlock / 64) {
        const int rt = item % n_rt, cg = item / n_rt;
        const int m = rt * 16 + l15;
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0, 0, 0, 0};
        for (int k0 = 0; k0 < K; k0 += 16) {
            const int k = k0 + 4 * lq;
            f32x4 b = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (m < nr && k + j < K) b[j] = stack_q_x(q, l, Elem<T>::to_f32(X[(size_t)m * pt + k + j]));
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                if (cg * 64 + nt * 16 >= P) break;                       // (wave-uniform)
                const int n = cg * 64 + nt * 16 + l15;
                f32x4 a = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n < P && k + j < K) a[j] = stack_q_w(q, l, W[(size_t)(k + j) * P + n]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[nt], 0, 0, 0);
            }
        }
        if (m >= nr) continue;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int n = cg * 64 + nt * 16 + 4 * lq;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < P) Wh[(size_t)m * pf + n + j] = qon ? finish_value<float>(acc[nt][j], 0, ep) : acc[nt][j];
        }
    }
}

// one stored entry of row i as a GAT layer sees it: its column in the group (-1: it leaves the group), its score E and
// whether it is live (values[e] > 0; under layer l's quantiser the quantised value, as stored in values_adj_q with
// SGX_QUANT_ADJ_DONE or quantised as it is read)
struct GatEntry { int c; float x; bool live; };
template <typename T, typename Q>
__device__ __forceinline__ GatEntry gat_entry(const GatGradArgs &a, const Q &q, int l, int e, int r0, int nr, float si,
                                              const float *__restrict__ s2, float alpha)
{
    GatEntry g = {a.col[e] - r0, 0.0f, false};
    if ((unsigned)g.c >= (unsigned)nr) {                              // (the plan admits no such edge)
        g.c = -1;
        return g;
    }
    g.x = leaky(si + s2[g.c], alpha);
    if constexpr (Q::kQuant) {
        if (q.on[l] && q.adj_done[l]) {
            g.live = q.val_q[e] > 0.0f;
            return g;
        }
    }
    g.live = stack_q_adj(q, l, Elem<T>::to_f32(static_cast<const T *>(a.val)[e])) > 0.0f;
    return g;
}

// the sum of v over the `lpr` lanes of a row (a power of two): the same bits in every lane
__device__ __forceinline__ float row_lanes_sum(float v, int lpr)
{
    for (int off = lpr >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, lpr);
    return v;
}

// Wh[0:nr][0:P] = fp32(X_l) . W_l for the group: a sparse layer 0 by the fma chain in CSR order, every other layer on the
// matrix cores.  With layer l's quantiser on: H_q = requant(X_q . W_q) as stack_form_h forms it in the forward.
template <typename T, typename Q>
__device__ __forceinline__ void gat_form_wh(const GatGradArgs &a, int l, int r0, int nr, const T *__restrict__ XD,
                                            float *__restrict__ Wh, const FeaRows &fr, const Q &q)
{
    const int K = a.K[l], P = a.P[l], pf = a.pitch_f, pt = a.pitch_t;
    const int nch = (P + 3) / 4;
    const float *__restrict__ W = a.W[l];
    if (l == 0 && a.gemm0 == 0) {
        const bool qon = stack_q_on(q, l);
        const sgx_epilogue ep = stack_ep_h(q, l);
        const T *__restrict__ vf = static_cast<const T *>(a.val_f);
        for (int it = threadIdx.x; it < nr * nch; it += kBlock) {
            const int i = it / nch, c0 = (it - i * nch) * 4;
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const int e0 = fr.staged ? fr.lrow[i] : a.rowptr_f[r0 + i];
            const int e1 = fr.staged ? fr.lrow[i + 1] : a.rowptr_f[r0 + i + 1];
            for (int e = e0; e < e1; ++e) {
                const int k = fr.staged ? fr.lcol[e] : a.col_f[e];
                if ((unsigned)k >= (unsigned)K) continue;
                const float x = stack_q_x(q, l, fr.staged ? fr.lx[e] : Elem<T>::to_f32(vf[e]));
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (c0 + u < P) acc[u] = __builtin_fmaf(x, stack_q_w(q, l, W[(size_t)k * P + c0 + u]), acc[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (c0 + u < P) Wh[(size_t)i * pf + c0 + u] = qon ? finish_value<float>(acc[u], 0, ep) : acc[u];
        }
    } else {
        wh_dense_lds<T, Q>(XD, pt, nr, K, P, W, Wh, pf, q, l);
    }
}

// A GAT layer of the group: Wh, the scores and the row statistics formed again, then Gs = S . g (also to the caller's G,
// S and E), gs = T and the group's share of grad_attention added into the slice.  XD holds X_l (dense) on entry; the
// caller has put a __syncthreads behind the tiles' last writes and puts one behind this.  Under the layer's quantiser
// the scores and the mask are the quantised forward's; Wh is then formed again from the unquantised operands.
template <typename T, typename Q>
__device__ __forceinline__ void gat_grad_layer(const GatGradArgs &a, const Q &q, int l, int r0, int nr, float *__restrict__ Gs,
                                               float *__restrict__ gs, const T *__restrict__ XD, float *__restrict__ Wh,
                                               float *__restrict__ sc, const FeaRows &fr, float *__restrict__ slice, bool first)
{
    const int P = a.P[l], pf = a.pitch_f;
    const int nch = (P + 3) / 4;
    float *const s1 = sc, *const s2 = sc + a.rows, *const rm = sc + 2 * a.rows, *const ri = sc + 3 * a.rows;
    float *const rsum = sc + 4 * a.rows, *const g1s = sc + 5 * a.rows;
    const float alpha = a.alpha[l];

    // Wh = fp32(X_l) . W_l; under the layer's quantiser H_q, which the scores are formed from
    gat_form_wh<T, Q>(a, l, r0, nr, XD, Wh, fr, q);
    __syncthreads();

    // the two scores of every row
    const int t8 = threadIdx.x & (kGatScoreLanes - 1), row8 = threadIdx.x / kGatScoreLanes;
    {
        const float *__restrict__ att = a.att[l];
        for (int i = row8; i < nr; i += kBlock / kGatScoreLanes) {
            const float *h = Wh + (size_t)i * pf;
            float p1 = 0.0f, p2 = 0.0f;
            for (int j = t8; j < P; j += kGatScoreLanes) {
                p1 = __builtin_fmaf(h[j], stack_q_w(q, l, att[j]), p1);
                p2 = __builtin_fmaf(h[j], stack_q_w(q, l, att[P + j]), p2);
            }
            p1 = row_lanes_sum(p1, kGatScoreLanes);
            p2 = row_lanes_sum(p2, kGatScoreLanes);
            if (t8 == 0) {
                s1[i] = p1;
                s2[i] = p2;
            }
        }
    }
    __syncthreads();

    // the row statistics: m_i over the live entries, then 1 / sum exp(x - m_i); a row without a live entry keeps 0, 0
    for (int i = row8; i < nr; i += kBlock / kGatScoreLanes) {
        const int e0 = a.rowptr[r0 + i], e1 = a.rowptr[r0 + i + 1];
        const float si = s1[i];
        float m = -INFINITY;
        for (int e = e0 + t8; e < e1; e += kGatScoreLanes) {
            const GatEntry g = gat_entry<T>(a, q, l, e, r0, nr, si, s2, alpha);
            if (g.live) m = fmaxf(m, g.x);
        }
#pragma unroll
        for (int off = kGatScoreLanes / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kGatScoreLanes));
        float sum = 0.0f;
        if (m != -INFINITY) {                                          // (the same for the row's eight lanes)
            for (int e = e0 + t8; e < e1; e += kGatScoreLanes) {
                const GatEntry g = gat_entry<T>(a, q, l, e, r0, nr, si, s2, alpha);
                if (g.live) sum += __builtin_amdgcn_exp2f((g.x - m) * kGatLog2e);
            }
        }
        sum = row_lanes_sum(sum, kGatScoreLanes);
        if (t8 == 0) {
            rm[i] = m != -INFINITY ? m : 0.0f;
            ri[i] = sum > 0.0f ? 1.0f / sum : 0.0f;
        }
    }
    // H_q is dead behind the scores' barrier: the unquantised Wh over the same tile, for d_e, T and sum g1 Wh
    if (stack_q_on(q, l)) gat_form_wh<T, StackPlain>(a, l, r0, nr, XD, Wh, fr, StackPlain());
    __syncthreads();

    // `lpr` lanes per row (a power of two, one lane per four columns); the weights of lpr entries at a time are formed one
    // per lane and read round the group, as in the forward's aggregate
    int lpr = 1;
    while (lpr < nch) lpr <<= 1;                                        // <= 64: P <= 256
    const int t = threadIdx.x & (lpr - 1), c0 = 4 * t;
    float *__restrict__ Gout = a.G[l], *__restrict__ Sout = a.S[l], *__restrict__ Eout = a.E[l];

    // pass 1: G_i = sum_e S_e g_c and rs_i = sum_e S_e (g_i . Wh_c)
    for (int i = threadIdx.x / lpr; i < nr; i += kBlock / lpr) {
        const int e0 = a.rowptr[r0 + i], e1 = a.rowptr[r0 + i + 1];
        const float si = s1[i], m = rm[i], inv = ri[i];
        float gi[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 4; ++u) gi[u] = c0 + u < P ? gs[(size_t)i * pf + c0 + u] : 0.0f;
        float rs = 0.0f;
        for (int base = e0; base < e1; base += lpr) {
            int c = -1;
            float w = 0.0f;
            if (base + t < e1) {
                const GatEntry g = gat_entry<T>(a, q, l, base + t, r0, nr, si, s2, alpha);
                if (g.live) {
                    c = g.c;
                    w = __builtin_amdgcn_exp2f((g.x - m) * kGatLog2e) * inv;
                }
                if (Sout) Sout[base + t] = w;
                if (Eout) Eout[base + t] = g.x;
            }
            const int n = e1 - base < lpr ? e1 - base : lpr;
            for (int j = 0; j < n; ++j) {
                const int cj = __shfl(c, j, lpr);
                const float wj = __shfl(w, j, lpr);
                if (cj < 0) continue;                                   // (the same for the row's lanes)
                float d = 0.0f;
                if (c0 < P) {
                    const f32x4 h = *reinterpret_cast<const f32x4 *>(Wh + (size_t)cj * pf + c0);
                    const f32x4 gc = *reinterpret_cast<const f32x4 *>(gs + (size_t)cj * pf + c0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (c0 + u < P) d = __builtin_fmaf(gi[u], h[u], d);
                        acc[u] = __builtin_fmaf(wj, gc[u], acc[u]);
                    }
                }
                d = row_lanes_sum(d, lpr);
                rs = __builtin_fmaf(wj, d, rs);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u >= P) break;
            Gs[(size_t)i * pf + c0 + u] = acc[u];
            if (Gout) Gout[(int64_t)(r0 + i) * P + c0 + u] = acc[u];
        }
        if (t == 0) rsum[i] = rs;
    }
    __syncthreads();                                                    // every row has read its neighbours' g

    // pass 2: sg_e = (S_e d_e - S_e rs_i) slope_e, g1_i = sum_e sg_e, T_i = sum_e sg_e Wh_c over g_i's place
    for (int i = threadIdx.x / lpr; i < nr; i += kBlock / lpr) {
        const int e0 = a.rowptr[r0 + i], e1 = a.rowptr[r0 + i + 1];
        const float si = s1[i], m = rm[i], inv = ri[i], rs = rsum[i];
        float gi[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 4; ++u) gi[u] = c0 + u < P ? gs[(size_t)i * pf + c0 + u] : 0.0f;
        float g1 = 0.0f;
        for (int base = e0; base < e1; base += lpr) {
            int c = -1;
            float w = 0.0f, slope = 0.0f;
            if (base + t < e1) {
                const GatEntry g = gat_entry<T>(a, q, l, base + t, r0, nr, si, s2, alpha);
                if (g.live) {
                    c = g.c;
                    w = __builtin_amdgcn_exp2f((g.x - m) * kGatLog2e) * inv;
                    slope = g.x > 0.0f ? 1.0f : alpha;
                }
            }
            const int n = e1 - base < lpr ? e1 - base : lpr;
            for (int j = 0; j < n; ++j) {
                const int cj = __shfl(c, j, lpr);
                const float wj = __shfl(w, j, lpr), slj = __shfl(slope, j, lpr);
                if (cj < 0) continue;
                f32x4 h = {0, 0, 0, 0};
                float d = 0.0f;
                if (c0 < P) {
                    h = *reinterpret_cast<const f32x4 *>(Wh + (size_t)cj * pf + c0);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (c0 + u < P) d = __builtin_fmaf(gi[u], h[u], d);
                }
                d = row_lanes_sum(d, lpr);
                const float sg = (wj * d - wj * rs) * slj;
                g1 += sg;
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(sg, h[u], acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u >= P) break;
            gs[(size_t)i * pf + c0 + u] = acc[u];                       // (only this row's lanes read g_i in this pass)
        }
        if (t == 0) g1s[i] = g1;
    }
    __syncthreads();

    // grad_attention += [sum_i g1_i Wh_i ; sum_i T_i], rows in order, the slice's previous value first
    float *__restrict__ ga = slice + a.aoff[l];
    for (int it = threadIdx.x; it < 2 * P; it += kBlock) {
        const int p = it < P ? it : it - P;
        float s = first ? 0.0f : ga[it];
        if (it < P)
            for (int i = 0; i < nr; ++i) s = __builtin_fmaf(g1s[i], Wh[(size_t)i * pf + p], s);
        else
            for (int i = 0; i < nr; ++i) s += gs[(size_t)i * pf + p];
        ga[it] = s;
    }
}

template <typename T, typename Q>
__device__ __forceinline__ void gat_stack_backward_body(const GatGradArgs &a, const Q &q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char stack_lds[];
    float *const Gs = reinterpret_cast<float *>(stack_lds);                // G_l = P . g_l   [rows][pitch_f]
    float *const gs = Gs + (size_t)a.rows * a.pitch_f;                      // g_l, then T_l    [rows][pitch_f]
    T *const XD = reinterpret_cast<T *>(gs + (size_t)a.rows * a.pitch_f);   // X_l = D_{l-1}    [rows][pitch_t]
    float *const Wh = reinterpret_cast<float *>(XD + (size_t)a.rows * a.pitch_t);   // X_l . W_l  [rows][pitch_f]
    float *const sc = Wh + (size_t)a.rows * a.pitch_f;                      // s1, s2, m, 1/l, rs, g1   [6][rows]
    const int pf = a.pitch_f, pt = a.pitch_t;
    const int L = a.n_layers;
    const T *__restrict__ val = static_cast<const T *>(a.val);
    float *const slice = a.ws + (size_t)blockIdx.x * a.slice;
    // sparse layer 0 of at most kGatSparseRegK columns: thread p keeps dW_0[0..K-1][p] in registers over all its groups
    const bool sparse_reg = a.gemm0 == 0 && a.K[0] <= kGatSparseRegK;
    float dw0[kGatSparseRegK];
#pragma unroll
    for (int k = 0; k < kGatSparseRegK; ++k) dw0[k] = 0.0f;

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
            // X_l into LDS (D_l, which it replaces, has already masked g_l); a CSR layer 0 puts the group's feature
            // entries there instead (rebased row offsets, columns, fp32 values) when they fit
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
            if (a.gat[l]) {
                __syncthreads();
                gat_grad_layer<T, Q>(a, q, l, r0, nr, Gs, gs, XD, Wh, sc, FeaRows{staged, lrow, lcol, lx}, slice, first);
            } else {
                // G = A . g: sgx_stack_backward's chain -- rows of A from global, g gathered from LDS
                const int nch = (P + 3) / 4;
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
                __syncthreads();
            }

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
                            if ((unsigned)k >= (unsigned)K) continue;
                            const float x = staged ? lx[e] : Elem<T>::to_f32(vf[e]);
                            if (sparse_reg) {
#pragma unroll
                                for (int kk = 0; kk < kGatSparseRegK; ++kk)
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

            // g_{l-1} = dtype(G_l . W_l^T) on the matrix cores (sgx_xw_dense's fp32 layout), masked by D_{l-1} = X_l;
            // a GAT layer's column sums above still read T from g's tile
            if (l > 0) {
                if (a.gat[l]) __syncthreads();
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
            for (int kk = 0; kk < kGatSparseRegK; ++kk)
                if (kk == k) v = dw0[kk];
            dw[(size_t)k * a.P[0] + threadIdx.x] = v;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gat_stack_backward_kernel(GatGradArgs a)
{
    gat_stack_backward_body<T>(a, StackPlain());
}

// the same launch with the layers' quantisers (fp32 only, stack_quant_bwd.hip)
template <typename T>
__global__ __launch_bounds__(kBlock) void quant_stack_backward_kernel(GatGradArgs a, StackQuantGrad q)
{
    gat_stack_backward_body<T>(a, q);
}

// a slice's blocks: grad_W of every layer, then grad_attention of every GAT layer
struct GatGradOut {
    int n, off[2 * kMaxLayers + 1], size[2 * kMaxLayers];
    float *out[2 * kMaxLayers];
};

// every gradient = the slices added in slice order (the first added to 0)
__global__ __launch_bounds__(kBlock) void gat_stack_grad_reduce_kernel(int n_slices, int slice, const float *__restrict__ ws,
                                                                       GatGradOut o)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= o.off[o.n]) return;
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
    int b = 0;
    while (b + 1 < o.n && idx >= o.off[b + 1]) ++b;
    if (idx - o.off[b] < o.size[b]) o.out[b][idx - o.off[b]] = s;          // (not the padding after a block)
}

// Desc: sgx_gat_stack_grad_desc or sgx_quant_stack_grad_desc (the same fields, field for field)
template <typename Desc>
int check_gat_grad(const Desc *d)
{
    int rc = stack_check_head(d);
    if (rc != SGX_OK) return rc;
    for (int l = 0; l < d->n_layers; ++l) {
        const auto &L = d->layer[l];
        if ((rc = stack_check_layer_shape(d, l)) != SGX_OK) return rc;
        if (!L.W || !L.grad_W) return SGX_ERR_NULL;
        if ((l < d->n_layers - 1 || L.relu) && !L.D && d->n_rows > 0) return SGX_ERR_NULL;
        if (L.gat_mode != 0 && L.gat_mode != 1) return SGX_ERR_UNSUPPORTED;
        if (L.gat_mode == 1 && (!L.attention || !L.grad_attention)) return SGX_ERR_NULL;
    }
    if (d->n_graphs > 0 && !d->grad_pooled) return SGX_ERR_NULL;
    return stack_check_batch(d);
}

// bytes of dynamic LDS: sgx_stack_backward's three tiles, the Wh tile and the six row arrays
size_t gat_grad_lds(int dtype, int max_width, int rows)
{
    return (size_t)rows * ((size_t)grad_row_bytes(dtype, max_width) + sizeof(float) * lds_pitch(SGX_F32, max_width) +
                           sizeof(float) * kGatRowFloats);
}

// what the call takes: a backward plan that fits, widths within it, tiles within a workgroup's LDS
template <typename Desc>
int gat_grad_supported(const Desc *d)
{
    const sgx_batch_plan *p = d->plan;
    if (p->kind != SGX_BATCH_BACKWARD || p->dtype != d->dtype || !p->fits || p->rows < 1 || p->max_width > kStackMaxWidth)
        return SGX_ERR_UNSUPPORTED;
    if (p->n_rows > 0 && p->n_groups < 1) return SGX_ERR_UNSUPPORTED;
    if (gat_grad_lds(d->dtype, p->max_width, p->rows) > kGatLdsLimit) return SGX_ERR_UNSUPPORTED;
    return stack_widths_fit(d) ? SGX_OK : SGX_ERR_UNSUPPORTED;
}

int gat_grad_grid(const sgx_batch_plan *p) { return p->n_groups < 1 ? 1 : (p->n_groups < kGatGradGrid ? p->n_groups : kGatGradGrid); }

// floats per slice, every block starting on 16 bytes; off / aoff: where the layers' blocks start
template <typename Desc>
size_t gat_grad_slice(const Desc *d, int *off, int *aoff)
{
    size_t n = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        if (off) off[l] = (int)n;
        n += ((size_t)d->layer[l].M_fea * d->layer[l].P_w + 3) / 4 * 4;
    }
    for (int l = 0; l < d->n_layers; ++l) {
        if (aoff) aoff[l] = (int)n;
        if (d->layer[l].gat_mode == 1) n += ((size_t)2 * d->layer[l].P_w + 3) / 4 * 4;
    }
    return n;
}

template <typename Desc>
size_t gat_grad_workspace(const Desc *d)
{
    return sgx_align_up((size_t)gat_grad_grid(d->plan) * gat_grad_slice(d, nullptr, nullptr) * sizeof(float), 256);
}

// kernel: gat_stack_backward_kernel<T> or quant_stack_backward_kernel<float>; optin: that kernel's; extra: what follows
// GatGradArgs in its arguments
template <typename Kernel, typename... Extra>
int launch_gat_backward(Kernel kernel, sgx_lds_optin &optin, const GatGradArgs &a, int grid, size_t lds, hipStream_t s,
                        const Extra &...extra)
{
    if (lds > (size_t)kStackLds) {
        const int rc = sgx_raise_dynamic_lds(kernel, optin, kGatLdsLimit);
        if (rc != SGX_OK) return rc;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, a, extra...);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

// launch(a, grid, lds): the descriptor's kernel
template <typename Desc, typename Launch>
int run_gat_backward(const Desc *d, hipStream_t s, Launch launch)
{
    const sgx_batch_plan *p = d->plan;
    GatGradArgs a;
    a.n_layers = d->n_layers;
    a.gemm0 = d->layer[0].gemm_mode;
    a.pitch_t = lds_pitch(d->dtype, p->max_width);
    a.pitch_f = lds_pitch(SGX_F32, p->max_width);
    a.rows = p->rows;
    a.n_groups = p->n_groups;
    int aoff[kMaxLayers];
    a.slice = (int)gat_grad_slice(d, a.off, aoff);
    GatGradOut o;
    o.n = 0;
    for (int l = 0; l < kMaxLayers; ++l) {
        const bool live = l < d->n_layers;
        const auto &L = d->layer[live ? l : 0];
        const bool gat = live && L.gat_mode == 1;
        a.relu[l] = live ? (L.relu ? 1 : 0) : 0;
        a.K[l] = live ? L.M_fea : 0;
        a.P[l] = live ? L.P_w : 0;
        if (!live) a.off[l] = a.slice;
        a.gat[l] = gat ? 1 : 0;
        a.aoff[l] = gat ? aoff[l] : a.slice;
        a.alpha[l] = gat ? L.alpha : 0.0f;
        a.W[l] = live ? L.W : nullptr;
        a.att[l] = gat ? L.attention : nullptr;
        a.D[l] = live ? L.D : nullptr;
        a.ldd[l] = live ? layer_ldd(L) : 0;
        a.G[l] = live ? L.G : nullptr;
        a.S[l] = gat ? L.S : nullptr;
        a.E[l] = gat ? L.E : nullptr;
    }
    for (int l = 0; l < d->n_layers; ++l) {
        o.off[o.n] = a.off[l];
        o.size[o.n] = d->layer[l].M_fea * d->layer[l].P_w;
        o.out[o.n++] = d->layer[l].grad_W;
    }
    for (int l = 0; l < d->n_layers; ++l) {
        if (!a.gat[l]) continue;
        o.off[o.n] = a.aoff[l];
        o.size[o.n] = 2 * d->layer[l].P_w;
        o.out[o.n++] = d->layer[l].grad_attention;
    }
    o.off[o.n] = o.off[o.n - 1] + o.size[o.n - 1];       // the reduction reads up to the last block's end
    for (int b = o.n; b < 2 * kMaxLayers; ++b) {
        o.off[b + 1] = o.off[o.n];
        o.size[b] = 0;
        o.out[b] = nullptr;
    }
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
    const int grid = gat_grad_grid(p);
    const size_t lds = gat_grad_lds(d->dtype, p->max_width, p->rows);
    const int rc = launch(a, grid, lds);
    if (rc != SGX_OK) return rc;
    hipLaunchKernelGGL(gat_stack_grad_reduce_kernel, dim3((unsigned)((o.off[o.n] + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       grid, a.slice, a.ws, o);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

// the entry point behind its own checks: workspace, the empty batch, the launch
template <typename Desc, typename Launch>
int gat_backward_entry(const Desc *d, hipStream_t s, Launch launch)
{
    if (!d->workspace || d->workspace_bytes < gat_grad_workspace(d)) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)d->workspace % 256 != 0) return SGX_ERR_ALIGN;
    if (d->n_rows == 0) {
        // no rows: every gradient is 0 (and there is no G, S or E to write)
        for (int l = 0; l < d->n_layers; ++l) {
            const auto &L = d->layer[l];
            SGX_HIP_CHECK(hipMemsetAsync(L.grad_W, 0, sizeof(float) * (size_t)L.M_fea * L.P_w, s));
            if (L.gat_mode == 1) SGX_HIP_CHECK(hipMemsetAsync(L.grad_attention, 0, sizeof(float) * 2 * (size_t)L.P_w, s));
        }
        return SGX_OK;
    }
    return run_gat_backward(d, s, launch);
}

}  // namespace
