// What the small-graph stack's files share.  With all of them (stack_plan.hip: sgx_batch_plan_*; stack.hip: sgx_stack_forward;
// stack_bwd.hip: sgx_stack_backward; stack_gat.hip: sgx_gat_stack_forward; stack_quant.hip: sgx_quant_stack_forward): the batch
// plan and its row budget, the LDS tiles' pitch, a workgroup's group of graphs (stack_group), the matrix-core X.W on an LDS
// tile, and the descriptor checks common to the forward and the backward descriptors (stack_check_*, stack_widths_fit).
// With the three forward files: the stages of the forward kernel, check_stack_desc and the chained path.
#pragma once
#include "sgx_device.h"
#include "quant_device.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f16x8 f16x8_u __attribute__((aligned(2)));
typedef f32x4 f32x4_u __attribute__((aligned(4)));

struct sgx_batch_plan {
    int dtype, n_rows, n_graphs, max_width;
    int rows;            // row budget R
    int n_groups;        // 0 when a graph is over R (or max_width over the fused kernel's limit)
    int max_graph;
    int fits;
    int kind;            // SGX_BATCH_FORWARD / SGX_BATCH_BACKWARD: which kernel's LDS tiles set the row budget
    int32_t *group_graph;   // [n_groups + 1] device: first graph of every group, then n_graphs
    int owns_groups;        // 0: group_graph is the caller's buffer (sgx_batch_plan_create_known), not freed here
};

#ifndef SGX_STACK_ROWS_CAP
// rows per group at most: smaller groups leave LDS for more workgroups per CU to hide the global reads' latency (a
// million MUTAG graphs, fp16, 64 wide: 224 rows / 2 workgroups per CU 11.9 ms, 128 / 4: 7.6 ms, 64: 7.8 ms)
#define SGX_STACK_ROWS_CAP 128
#endif

namespace {

constexpr int kStackLds = 64 * 1024;   // bytes of LDS per workgroup: two workgroups per CU (160 KiB)
constexpr int kStackMaxWidth = 256;
constexpr int kMaxLayers = 4;

// LDS row pitch in elements: 16-byte fragments, plus 16 bytes so that consecutive rows start on different banks
inline int lds_pitch(int dtype, int width)
{
    const int per16 = (int)(16 / sgx_elem_size(dtype));
    return (width + per16 - 1) / per16 * per16 + per16;
}

// the backward kernel's tiles: X_l / D in dtype, g and G in fp32
inline int grad_row_bytes(int dtype, int max_width)
{
    return lds_pitch(dtype, max_width) * (int)sgx_elem_size(dtype) + 2 * lds_pitch(SGX_F32, max_width) * (int)sizeof(float);
}

inline int rows_budget(int dtype, int max_width, int kind)
{
    if (max_width < 1 || max_width > kStackMaxWidth) return 0;
    const int row_bytes = kind == SGX_BATCH_BACKWARD ? grad_row_bytes(dtype, max_width)
                                                     : 2 * lds_pitch(dtype, max_width) * (int)sgx_elem_size(dtype);   // X/D + H
    const int rows = kStackLds / row_bytes / 16 * 16;                                         // whole 16-row MFMA tiles
    return rows < SGX_STACK_ROWS_CAP ? rows : SGX_STACK_ROWS_CAP;
}

// graphs [gf, gl) = rows [r0, r0 + nr) of the batch: group `grp` of the plan.  Empty (gf >= gl, nr = 0) when the group has
// no graph or more rows than the tiles (the plan never makes such a group).
struct StackGroup { int gf, gl, r0, nr; };
__device__ __forceinline__ StackGroup stack_group(const int32_t *group_graph, const int32_t *graph_ptr, int rows, int grp)
{
    StackGroup g = {group_graph[grp], group_graph[grp + 1], 0, 0};
    if (g.gf < g.gl) {
        g.r0 = graph_ptr[g.gf];
        g.nr = graph_ptr[g.gl] - g.r0;
    }
    if (g.nr > rows) g = {g.gf, g.gf, g.r0, 0};
    return g;
}

// ---- the forward kernel's arguments and stages ----------------------------------------------------------------------
struct StackArgs {
    int n_layers, gemm0, C, pitch;
    int relu[kMaxLayers], K[kMaxLayers], P[kMaxLayers];
    const void *B[kMaxLayers];
    void *D[kMaxLayers];
    int64_t ldd[kMaxLayers];
    const int32_t *graph_ptr, *group_graph;
    const int32_t *rowptr, *col;
    const void *val;
    const int32_t *rowptr_f, *col_f;
    const void *val_f;
    const float *W_head, *bias;
    float *pooled, *logits;
    int rows;
};

// What a layer's quantiser (sgx_quant) does inside the stages, as a policy of the stage templates.  StackPlain: nothing --
// every hook below is compiled out, so the plain kernels keep their code.  StackQuant (fp32 only, sgx_quant_stack_forward):
// per layer the operand grids (W and the attention vector signed, X and the adjacency values unsigned, one
// fake_quantize_value per element as it is read) and the two store epilogues of sgx_layer_forward.
struct StackPlain {
    static constexpr bool kQuant = false;
};
struct StackQuant {
    static constexpr bool kQuant = true;
    int on[kMaxLayers];          // the layer has a quantiser; every other field of an `off` layer is unused
    int qbits[kMaxLayers];
    int adj_done[kMaxLayers];    // SGX_QUANT_ADJ_DONE: the adjacency values are taken as stored
    float inv_fea[kMaxLayers], zero_fea[kMaxLayers], inv_w[kMaxLayers], zero_w[kMaxLayers], inv_adj[kMaxLayers],
        zero_adj[kMaxLayers];
    sgx_epilogue ep_h[kMaxLayers], ep_d[kMaxLayers];
};

// a weight or an attention element of layer l
template <typename Q> __device__ __forceinline__ float stack_q_w(const Q &q, int l, float v)
{
    if constexpr (Q::kQuant) {
        if (q.on[l]) return sgx_quantizer::fake_quantize_value(1, q.qbits[l], q.inv_w[l], q.zero_w[l], v);
    }
    return v;
}
// an element of X_l
template <typename Q> __device__ __forceinline__ float stack_q_x(const Q &q, int l, float v)
{
    if constexpr (Q::kQuant) {
        if (q.on[l]) return sgx_quantizer::fake_quantize_value(0, q.qbits[l], q.inv_fea[l], q.zero_fea[l], v);
    }
    return v;
}
// a stored adjacency value as layer l reads it
template <typename Q> __device__ __forceinline__ float stack_q_adj(const Q &q, int l, float v)
{
    if constexpr (Q::kQuant) {
        if (q.on[l] && !q.adj_done[l]) return sgx_quantizer::fake_quantize_value(0, q.qbits[l], q.inv_adj[l], q.zero_adj[l], v);
    }
    return v;
}
// the epilogues of layer l's two stores (none for a plain layer)
template <typename Q> __device__ __forceinline__ sgx_epilogue stack_ep_h(const Q &q, int l)
{
    if constexpr (Q::kQuant) {
        if (q.on[l]) return q.ep_h[l];
    }
    return sgx_epilogue{0.0f, 0.0f, 0.0f, 0.0f};
}
template <typename Q> __device__ __forceinline__ sgx_epilogue stack_ep_d(const Q &q, int l)
{
    if constexpr (Q::kQuant) {
        if (q.on[l]) return q.ep_d[l];
    }
    return sgx_epilogue{0.0f, 0.0f, 0.0f, 0.0f};
}
// what the aggregate of layer l leaves in the X tile for D_l = v: X_{l+1} on layer l + 1's feature grid where that layer
// has a quantiser (the caller's D gets v itself; the last layer's tile stays as it is for the readout)
template <typename T, typename Q> __device__ __forceinline__ T stack_next_x(const Q &q, int l, int n_layers, T v)
{
    if constexpr (Q::kQuant && sizeof(T) == 4) {
        if (l + 1 < n_layers) return stack_q_x(q, l + 1, v);
    }
    return v;
}

template <typename T> struct Mfma;

// fp16: a k-step of 32; lane quad lq holds k = k0 + 8 lq .. + 7 of its row (xw_dense_f16_kernel's layout)
template <> struct Mfma<f16> {
    static constexpr int kStep = 32;
    typedef f16x8 frag;
    static __device__ __forceinline__ frag load(const f16 *row, int k, int k_end, bool ok)
    {
        frag v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (!ok) return v;
        if (k + 8 <= k_end) return *reinterpret_cast<const f16x8_u *>(row + k);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k + j < k_end) v[j] = row[k + j];
        return v;
    }
    static __device__ __forceinline__ int lane_k(int k0, int lq) { return k0 + 8 * lq; }
    static __device__ __forceinline__ f32x4 step(frag a, frag b, f32x4 acc)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
    }
};

// fp32: a k-block of 16; lane quad lq holds k = k0 + 4 lq .. + 3, step j of the block consumes element j
// (xw_dense_f32_kernel's layout and step order)
template <> struct Mfma<float> {
    static constexpr int kStep = 16;
    typedef f32x4 frag;
    static __device__ __forceinline__ frag load(const float *row, int k, int k_end, bool ok)
    {
        frag v = {0, 0, 0, 0};
        if (!ok) return v;
        if (k + 4 <= k_end) return *reinterpret_cast<const f32x4_u *>(row + k);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k + j < k_end) v[j] = row[k + j];
        return v;
    }
    static __device__ __forceinline__ int lane_k(int k0, int lq) { return k0 + 4 * lq; }
    static __device__ __forceinline__ f32x4 step(frag a, frag b, f32x4 acc)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
        return acc;
    }
};

// H[0:nr][0:P] = X[0:nr][0:K] . Wt^T, X in LDS, Wt [P][K] in global.  A wavefront takes (16-row tile, 64-column
// group) items: the MFMA forms the transposed tile H^T = Wt . X^T as in xw_dense.hip, so a lane ends with four
// consecutive columns of one row, handed to store(m, n, fp32 sum).
// q, l: the quantiser of W (layer l's signed grid on every element the operand load brings in; pad elements stay 0).
template <typename T, typename Store, typename Q = StackPlain>
__device__ __forceinline__ void xw_dense_lds_apply(const T *__restrict__ X, int pitch, int nr, int K, int P,
                                                   const T *__restrict__ Wt, Store store, const Q &q = Q(), int l = 0)
{
    typedef Mfma<T> M;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int l15 = lane & 15, lq = lane >> 4;
    const int n_rt = (nr + 15) / 16, n_cg = (P + 63) / 64;
    for (int item = wave; item < n_rt * n_cg; item += kBlock / 64) {
        const int rt = item % n_rt, cg = item / n_rt;
        const int m = rt * 16 + l15;
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0, 0, 0, 0};
        for (int k0 = 0; k0 < K; k0 += M::kStep) {
            const int k = M::lane_k(k0, lq);
            const typename M::frag b = M::load(X + (size_t)m * pitch, k, K, m < nr);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                if (cg * 64 + nt * 16 >= P) break;                       // (wave-uniform)
                const int n = cg * 64 + nt * 16 + l15;
                typename M::frag a = M::load(Wt + (size_t)n * K, k, K, n < P);
                if constexpr (Q::kQuant && sizeof(T) == 4) {
                    if (q.on[l] && n < P) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (k + j < K) a[j] = stack_q_w(q, l, a[j]);
                    }
                }
                acc[nt] = M::step(a, b, acc[nt]);
            }
        }
        if (m >= nr) continue;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int n = cg * 64 + nt * 16 + 4 * lq;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < P) store(m, n + j, acc[nt][j]);
        }
    }
}

template <typename T, typename Q = StackPlain>
__device__ __forceinline__ void xw_dense_lds(const T *__restrict__ X, T *__restrict__ H, int pitch, int nr, int K, int P,
                                             const T *__restrict__ Wt, const Q &q = Q(), int l = 0)
{
    if constexpr (Q::kQuant && sizeof(T) == 4) {
        // H = requant(X_q . W_q): the epilogue sgx_xw_dense applies on its stores
        const sgx_epilogue ep = stack_ep_h(q, l);
        xw_dense_lds_apply<T>(X, pitch, nr, K, P, Wt,
                              [&](int m, int n, float v) { H[(size_t)m * pitch + n] = finish_value<T>(v, 0, ep); }, q, l);
    } else {
        xw_dense_lds_apply<T>(X, pitch, nr, K, P, Wt,
                              [&](int m, int n, float v) { H[(size_t)m * pitch + n] = Elem<T>::from_f32(v); });
    }
}

// Stage 1 of layer l for the group of rows [r0, r0 + nr): Hs = dtype(X_l . W_l), X_l = XD (layers >= 1) or the caller's
// features.  The caller puts a __syncthreads behind it.  With a quantiser: layer 0's features go to their grid as they are
// read (CSR entries) or copied into LDS (dense rows), W as it is read, H through the re-quantisation on its store; the
// X tile of a layer >= 1 is already on its grid (stack_next_x).
template <typename T, typename Q = StackPlain>
__device__ __forceinline__ void stack_form_h(const StackArgs &a, int l, int r0, int nr, T *__restrict__ XD, T *__restrict__ Hs,
                                             const Q &q = Q())
{
    const int K = a.K[l], P = a.P[l], pitch = a.pitch;
    const T *__restrict__ Wt = static_cast<const T *>(a.B[l]);
    const int nch = (P + 3) / 4;                                // four columns per thread in the row-wise stages
    if (l == 0 && a.gemm0 == 0) {
        // H = X.W for a CSR X: per (row, column) an fp32 fma chain over the row's entries in CSR order
        const T *__restrict__ vf = static_cast<const T *>(a.val_f);
        for (int it = threadIdx.x; it < nr * nch; it += kBlock) {
            const int i = it / nch, c0 = (it - i * nch) * 4;
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const int e0 = a.rowptr_f[r0 + i], e1 = a.rowptr_f[r0 + i + 1];
            for (int e = e0; e < e1; ++e) {
                const int k = a.col_f[e];
                if ((unsigned)k >= (unsigned)K) continue;          // (the chained gather reads 0 there)
                const float x = stack_q_x(q, l, Elem<T>::to_f32(vf[e]));
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (c0 + u < P)
                        acc[u] = __builtin_fmaf(x, stack_q_w(q, l, Elem<T>::to_f32(Wt[(size_t)(c0 + u) * K + k])), acc[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u >= P) continue;
                if constexpr (Q::kQuant && sizeof(T) == 4) Hs[(size_t)i * pitch + c0 + u] = finish_value<T>(acc[u], 0, stack_ep_h(q, l));
                else Hs[(size_t)i * pitch + c0 + u] = Elem<T>::from_f32(acc[u]);
            }
        }
    } else {
        if (l == 0) {
            // dense layer-0 rows of the group into LDS
            const T *__restrict__ X = static_cast<const T *>(a.val_f) + (size_t)r0 * K;
            for (int it = threadIdx.x; it < nr * K; it += kBlock) {
                const int i = it / K, k = it - i * K;
                if constexpr (Q::kQuant && sizeof(T) == 4) XD[(size_t)i * pitch + k] = stack_q_x(q, l, X[it]);
                else XD[(size_t)i * pitch + k] = X[it];
            }
            __syncthreads();
        }
        xw_dense_lds<T, Q>(XD, Hs, pitch, nr, K, P, Wt, q, l);
    }
}

// Stage 2, the GCN form: XD = D_l = act(A . H_l), rows of A from global, columns rebased to the group's first row, H
// gathered from LDS; also to the caller's D when asked.  The caller puts a __syncthreads behind it.  With a quantiser: the
// adjacency values on their grid as they are read, D = act(sum) * deq_factor, the X tile through stack_next_x.
template <typename T, typename Q = StackPlain>
__device__ __forceinline__ void stack_gcn_aggregate(const StackArgs &a, int l, int r0, int nr, T *__restrict__ XD,
                                                    const T *__restrict__ Hs, const Q &q = Q())
{
    const int P = a.P[l], pitch = a.pitch;
    const int nch = (P + 3) / 4;
    const sgx_epilogue ep = stack_ep_d(q, l);
    const T *__restrict__ val = static_cast<const T *>(a.val);
    T *__restrict__ Dg = static_cast<T *>(a.D[l]);
    const int64_t ldd = a.ldd[l];
    const int relu = a.relu[l];
    for (int it = threadIdx.x; it < nr * nch; it += kBlock) {
        const int i = it / nch, c0 = (it - i * nch) * 4;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int e0 = a.rowptr[r0 + i], e1 = a.rowptr[r0 + i + 1];
        for (int e = e0; e < e1; ++e) {
            const int c = a.col[e] - r0;
            if ((unsigned)c >= (unsigned)nr) continue;         // (the plan admits no such edge)
            const float w = stack_q_adj(q, l, Elem<T>::to_f32(val[e]));
            const T *h = Hs + (size_t)c * pitch + c0;
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(w, Elem<T>::to_f32(h[u]), acc[u]);
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

// The readout of graphs [gf, gl) from XD = D_{n_layers-1}: one wavefront per graph; lane j of the row sums holds columns
// j, j + 64, ... -- the columns its head fmas read, so the means stay in registers
template <typename T>
__device__ __forceinline__ void stack_readout(const StackArgs &a, int gf, int gl, int r0, const T *__restrict__ XD)
{
    if (!a.pooled && !a.logits) return;
    const int pitch = a.pitch;
    const int F = a.P[a.n_layers - 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int g = gf + wave; g < gl; g += kBlock / 64) {
        const int s0 = a.graph_ptr[g] - r0, s1 = a.graph_ptr[g + 1] - r0;
        const float inv = s1 > s0 ? 1.0f / (float)(s1 - s0) : 0.0f;
        float mean[kStackMaxWidth / 64];
#pragma unroll
        for (int q = 0; q < kStackMaxWidth / 64; ++q) {
            const int j = lane + 64 * q;
            mean[q] = 0.0f;
            if (j < F) {
                float s = 0.0f;
                for (int r = s0; r < s1; ++r) s += Elem<T>::to_f32(XD[(size_t)r * pitch + j]);
                s *= inv;
                mean[q] = s;
                if (a.pooled) a.pooled[(int64_t)g * F + j] = s;
            }
        }
        if (!a.logits) continue;
        for (int c = 0; c < a.C; ++c) {
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < kStackMaxWidth / 64; ++q) {
                const int j = lane + 64 * q;
                if (j < F) s = __builtin_fmaf(a.W_head[(int64_t)c * F + j], mean[q], s);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) a.logits[(int64_t)g * a.C + c] = s + (a.bias ? a.bias[c] : 0.0f);
        }
    }
}

// ---- descriptor checks for the forward descriptors and sgx_stack_grad_desc alike; a caller's own go between them ------
template <typename Layer> int64_t layer_ldd(const Layer &L) { return L.ldd == 0 ? L.P_w : L.ldd; }

// the descriptor itself: layer count, dtype, the plan and its batch
template <typename Desc> int stack_check_head(const Desc *d)
{
    if (!d) return SGX_ERR_NULL;
    if (d->n_layers < 1 || d->n_layers > kMaxLayers) return SGX_ERR_SHAPE;
    if (d->dtype != SGX_F16 && d->dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    if (!d->plan) return SGX_ERR_NULL;
    if (d->n_rows != d->plan->n_rows || d->n_graphs != d->plan->n_graphs) return SGX_ERR_SHAPE;
    return SGX_OK;
}

// layer l's gemm_mode, widths and ldd
template <typename Desc> int stack_check_layer_shape(const Desc *d, int l)
{
    const auto &L = d->layer[l];
    if (L.gemm_mode != 0 && L.gemm_mode != 1) return SGX_ERR_UNSUPPORTED;
    if (l > 0 && L.gemm_mode != 1) return SGX_ERR_UNSUPPORTED;
    if (L.M_fea < 1 || L.P_w < 1 || L.ldd < 0 || (L.ldd != 0 && L.ldd < L.P_w)) return SGX_ERR_SHAPE;
    if (l > 0 && L.M_fea != d->layer[l - 1].P_w) return SGX_ERR_SHAPE;
    return SGX_OK;
}

// graph_ptr, the adjacency and the features of a batch that has any
template <typename Desc> int stack_check_batch(const Desc *d)
{
    if (d->n_graphs > 0 && !d->graph_ptr) return SGX_ERR_NULL;
    if (d->n_rows > 0) {
        if (!d->rowPtr_adj || !d->columnIndex_adj || !d->values_adj || !d->values_fea) return SGX_ERR_NULL;
        if (d->layer[0].gemm_mode == 0 && (!d->rowPtr_fea || !d->columnIndex_fea)) return SGX_ERR_NULL;
    }
    return SGX_OK;
}

// every width the kernels put into an LDS tile is within the plan's
template <typename Desc> bool stack_widths_fit(const Desc *d)
{
    for (int l = 0; l < d->n_layers; ++l) {
        const auto &L = d->layer[l];
        if (L.P_w > d->plan->max_width || ((l > 0 || L.gemm_mode == 1) && L.M_fea > d->plan->max_width)) return false;
    }
    return true;
}

// ---- the forward descriptors (sgx_stack_desc, sgx_gat_stack_desc, sgx_quant_stack_desc): checks and the chained path --
// layer_extra(L): what the descriptor's layer type adds to a layer's checks (SGX_OK for sgx_stack_layer)
template <typename Desc, typename LayerExtra>
int check_stack_desc(const Desc *d, LayerExtra layer_extra)
{
    int rc = stack_check_head(d);
    if (rc != SGX_OK) return rc;
    if (d->C < 0) return SGX_ERR_SHAPE;
    for (int l = 0; l < d->n_layers; ++l) {
        if ((rc = stack_check_layer_shape(d, l)) != SGX_OK) return rc;
        if (!d->layer[l].B) return SGX_ERR_NULL;
        if ((rc = layer_extra(d->layer[l])) != SGX_OK) return rc;
    }
    if (d->C > 0 && !d->W_head) return SGX_ERR_NULL;
    return stack_check_batch(d);
}

template <typename Desc>
bool stack_fused_applies(const Desc *d)
{
    const sgx_batch_plan *p = d->plan;
    if (!p->fits || p->n_groups < 1 || p->dtype != d->dtype || p->max_width > kStackMaxWidth) return false;
    return stack_widths_fit(d);
}

struct ChainCarve {
    size_t h_off, d_off, w_off, x_off, total;
    int64_t ld;          // pitch of H and of the intermediate D
};

// extra_bytes: what the descriptor's aggregates need beside H, D and W (at x_off; 0 for sgx_stack_desc)
template <typename Desc>
ChainCarve stack_chain_carve(const Desc *d, size_t extra_bytes)
{
    ChainCarve c;
    const size_t es = sgx_elem_size(d->dtype);
    int pmax = 1;
    for (int l = 0; l < d->n_layers; ++l) pmax = d->layer[l].P_w > pmax ? d->layer[l].P_w : pmax;
    c.ld = sgx_ldh(d->dtype, pmax);
    size_t off = 0;
    c.h_off = off; off += sgx_align_up((size_t)d->n_rows * c.ld * es, 256);
    c.d_off = off; off += sgx_align_up((size_t)d->n_rows * c.ld * es, 256);
    c.w_off = off;
    if (d->layer[0].gemm_mode == 0) off += sgx_align_up((size_t)d->layer[0].M_fea * sgx_ldh(d->dtype, d->layer[0].P_w) * es, 256);
    c.x_off = off; off += sgx_align_up(extra_bytes, 256);
    c.total = off;
    return c;
}

// the chain sgx_layer_forward x n_layers -> sgx_readout_mean_linear with the same kernels, no plans;
// aggregate(l, H, ldh, D, ldd): layer l's D = act(A . H) in the descriptor's form
template <typename Desc, typename Aggregate>
int stack_run_chain(const Desc *d, const ChainCarve &c, hipStream_t s, Aggregate aggregate)
{
    if (!d->workspace || d->workspace_bytes < c.total) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)d->workspace % 256 != 0) return SGX_ERR_ALIGN;
    char *ws = static_cast<char *>(d->workspace);
    void *H = ws + c.h_off;
    const void *X = d->values_fea;
    int64_t ldx = d->layer[0].M_fea;
    int rc;
    for (int l = 0; l < d->n_layers; ++l) {
        const auto &L = d->layer[l];
        if (l == 0 && L.gemm_mode == 0) {
            const int64_t ldw = sgx_ldh(d->dtype, L.P_w);
            void *W = ws + c.w_off;
            rc = sgx_transpose(d->dtype, L.P_w, L.M_fea, L.B, L.M_fea, W, ldw, s);              // B [P][M] -> W [M][ldw]
            if (rc != SGX_OK) return rc;
            rc = sgx_spmm_launch(d->dtype, SGX_ACC_F32, 1, /*relu*/0, d->n_rows, L.M_fea, L.P_w, d->rowPtr_fea,
                                 d->columnIndex_fea, d->values_fea, W, ldw, H, c.ld, nullptr, nullptr, 0, s, nullptr, nullptr,
                                 0, /*fea_stage*/true);
        } else {
            rc = sgx_xw_dense_ep(d->dtype, SGX_ACC_F32, 1, d->n_rows, L.M_fea, L.P_w, X, ldx, L.B, L.M_fea, H, c.ld, s,
                                 sgx_no_epilogue());
        }
        if (rc != SGX_OK) return rc;
        void *D = L.D ? L.D : ws + c.d_off;
        const int64_t ldd = L.D ? layer_ldd(L) : c.ld;
        rc = aggregate(l, H, c.ld, D, ldd);
        if (rc != SGX_OK) return rc;
        X = D;
        ldx = ldd;
    }
    float *logits = d->C > 0 ? d->logits : nullptr;
    if (!d->pooled && !logits) return SGX_OK;
    return sgx_readout_mean_linear(d->dtype, d->n_graphs, d->layer[d->n_layers - 1].P_w, logits ? d->C : 0, X, ldx,
                                   d->graph_ptr, d->W_head, d->bias, d->pooled, logits, s);
}

// the GCN aggregate of the chain: sgx_spmm_csr without a plan
template <typename Desc>
int stack_chain_gcn(const Desc *d, int l, const void *H, int64_t ldh, void *D, int64_t ldd, hipStream_t s)
{
    const auto &L = d->layer[l];
    return sgx_spmm_launch(d->dtype, SGX_ACC_F32, 1, L.relu ? 1 : 0, d->n_rows, d->n_rows, L.P_w, d->rowPtr_adj,
                           d->columnIndex_adj, d->values_adj, H, ldh, D, ldd, nullptr, nullptr, 0, s);
}

// the forward kernel's arguments from either descriptor
template <typename Desc>
StackArgs stack_args(const Desc *d)
{
    const sgx_batch_plan *p = d->plan;
    StackArgs a;
    a.n_layers = d->n_layers;
    a.gemm0 = d->layer[0].gemm_mode;
    a.C = d->logits ? d->C : 0;
    a.pitch = lds_pitch(d->dtype, p->max_width);
    a.rows = p->rows;
    for (int l = 0; l < kMaxLayers; ++l) {
        const bool live = l < d->n_layers;
        a.relu[l] = live ? (d->layer[l].relu ? 1 : 0) : 0;
        a.K[l] = live ? d->layer[l].M_fea : 0;
        a.P[l] = live ? d->layer[l].P_w : 0;
        a.B[l] = live ? d->layer[l].B : nullptr;
        a.D[l] = live ? d->layer[l].D : nullptr;
        a.ldd[l] = live ? layer_ldd(d->layer[l]) : 0;
    }
    a.graph_ptr = d->graph_ptr;
    a.group_graph = p->group_graph;
    a.rowptr = d->rowPtr_adj;
    a.col = d->columnIndex_adj;
    a.val = d->values_adj;
    a.rowptr_f = d->rowPtr_fea;
    a.col_f = d->columnIndex_fea;
    a.val_f = d->values_fea;
    a.W_head = d->W_head;
    a.bias = d->bias;
    a.pooled = d->pooled;
    a.logits = a.C > 0 ? d->logits : nullptr;
    return a;
}

}  // namespace
