// The classifier tail of a node-classification step in one call (sgx_node_loss, include/sgx.h "the node loss head"):
// dropout on the last layer's rows, the C x P Linear head, softmax cross entropy (mean over the SELECTED rows: a prefix,
// a byte mask, or both) and every gradient of it -- grad_H for the layers' backward, grad_W / grad_bias for the optimiser
// -- plus the selected rows' count and how many of them the arg-max gets right.  What GAT_PYNQ's training loop runs as
// F.dropout, self.lin, out[mask], CrossEntropyLoss and their autograd nodes.
//
// Three launches: the count M of selected rows (integers: a partial count per workgroup, stored plainly, which the later
// launches add up; gs = grad_scale / M needs it before any gradient); the main kernel; the reduction of its slices.  In
// the main kernel a workgroup owns the row blocks b = slice, slice + S, ... of SGX_NODE_LOSS_ROWS rows (S = min(n_blocks,
// SGX_NODE_LOSS_GRID) whatever the device).  A block none of whose rows is needed only zero-fills its grad_H rows.
// Otherwise the block's x = dropout(H), logits (tail_device.h: node_block_front, row_cross_entropy) and dz tiles live in
// LDS, and every thread keeps its C * P / 256 grad_W accumulators in registers across all the blocks of the slice; the
// slice's sums go to the workspace with plain stores and the last launch adds the slices in slice order.
// No floating-point atomics: the same bits on every run.
#include "tail_device.h"

using namespace sgx_tail;

namespace {

constexpr int kAcc = kMaxCP / kBlock;                       // grad_W accumulators a thread holds at most
constexpr int kCountPerThread = 16, kCountGrid = 256;
constexpr size_t kHeader = kCountGrid * sizeof(int64_t);    // the workspace begins with the count's partials

// parts[b] = the number of rows i < n_sel (= min(n_prefix, n_rows)) with mask[i] != 0 that workgroup b walks; M is their sum
__global__ __launch_bounds__(kBlock) void node_count_kernel(int64_t n_sel, const uint8_t *__restrict__ mask, int64_t *__restrict__ parts)
{
    __shared__ int wave_cnt[kBlock / 64];
    if (!mask) {
        if (blockIdx.x == 0 && threadIdx.x == 0) parts[0] = n_sel;
        return;
    }
    int cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_sel; i += stride) cnt += mask[i] != 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t n = 0;
        for (int w = 0; w < kBlock / 64; ++w) n += wave_cnt[w];
        parts[blockIdx.x] = n;
    }
}

__device__ __forceinline__ int64_t node_count_total(const int64_t *__restrict__ parts, int n_parts)
{
    int64_t M = 0;
    for (int k = 0; k < n_parts; ++k) M += parts[k];
    return M;
}

struct NodeArgs {
    NodeRows r;
    int64_t n_blocks;
    int S, n_parts;
    const int64_t *target;
    Dropout drop;
    uint64_t seed, step;
    const int64_t *step_dev;
    float grad_scale;
    float *grad_H;                    // NULL: evaluation mode, no gradient is formed
    const int64_t *parts;             // the count kernel's partial counts [n_parts]
    float *slices;                    // [S][C * P + C + 2]: grad_W, grad_bias, the loss sum, the correct count (an int's bits)
};

// NK: the grad_W accumulators a thread holds, ceil(C * P / 256) rounded up to 1, 4, 16 or 64 (the registers set how many
// workgroups share a CU)
template <int NK>
__global__ __launch_bounds__(kBlock) void node_loss_kernel(NodeArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char node_lds[];
    const int tid = threadIdx.x;
    const int P = a.r.P, C = a.r.C, CP = C * P, pitch = a.r.pitch_w;
    float *const Ws = reinterpret_cast<float *>(node_lds);  // [C][pitch]; the layout is node_loss_lds_bytes's
    float *const xs = Ws + (size_t)C * pitch;               // [kRows][P]
    float *const zs = xs + (size_t)kRows * P;               // [kRows][C]
    float *const dzs = zs + (size_t)kRows * C;              // [kRows][C]
    __shared__ float lse_s[kRows], part_s[kRows];
    __shared__ int tgt_s[kRows], corr_s[kRows];
    __shared__ unsigned sel_s[2];                           // by the parity of the iteration: a wave may still read the last one
    const bool grads = a.grad_H != nullptr;
    const uint64_t key = dropout_key(a.seed, a.step, a.step_dev);
    const float gs = a.grad_scale / (float)node_count_total(a.parts, a.n_parts);    // M == 0: no row is selected, gs is never used
    float acc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = 0.0f;
    float acc_b = 0.0f, loss_sum = 0.0f;                    // thread c's bias gradient; thread r's loss over its row of every block
    int correct = 0;
    bool w_ready = false;
    int it = 0;
    for (int64_t b = blockIdx.x; b < a.n_blocks; b += a.S, it ^= 1) {
        const NodeBlock blk = node_block_front<true>(a.r, b, it, w_ready, Ws, xs, zs, sel_s, key, a.drop);
        const int64_t base = blk.base;
        const int rows_here = blk.rows_here;
        const unsigned selbits = blk.selbits;
        if (blk.needbits == 0) {                             // nothing to compute: H is not read
            if (grads)
                for (int e = tid; e < rows_here * P; e += kBlock) a.grad_H[base * P + e] = 0.0f;
            continue;
        }
        if (tid < kRows) {
            int tgt = -1;
            if ((selbits >> tid) & 1u) {
                const float *z = zs + tid * C;
                const int64_t t = a.target[base + tid];
                const RowCe ce = row_cross_entropy(z, C, t);
                lse_s[tid] = ce.lse;
                if (ce.live) {
                    tgt = (int)t;
                    loss_sum = loss_sum + (ce.lse - z[t]);
                    correct += ce.best == tgt;
                }
            }
            tgt_s[tid] = tgt;
        }
        if (grads) {
            __syncthreads();
            for (int e = tid; e < kRows * C; e += kBlock) {
                const int r = e / C, c = e - r * C;
                float d = 0.0f;
                if (((selbits >> r) & 1u) && tgt_s[r] >= 0) d = (expf(zs[e] - lse_s[r]) - (c == tgt_s[r] ? 1.0f : 0.0f)) * gs;
                dzs[e] = d;
            }
            __syncthreads();
            for (int e = tid; e < rows_here * P; e += kBlock) {
                const int r = e / P, j = e - r * P;
                float v = 0.0f;
                if ((selbits >> r) & 1u) {
                    if (dropout_keep(key, base * P + e, a.drop.keep_from)) {
                        float s = 0.0f;
                        for (int c = 0; c < C; ++c) s = __builtin_fmaf(dzs[r * C + c], Ws[c * pitch + j], s);
                        v = a.drop.scale * s;
                    }
                }
                a.grad_H[base * P + e] = v;
            }
            if (selbits) {
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int e = tid + k * kBlock;
                    if (e < CP) {
                        const int c = e / P, j = e - c * P;
                        float s = acc[k];
                        for (int r = 0; r < kRows; ++r)
                            if ((selbits >> r) & 1u) s = __builtin_fmaf(dzs[r * C + c], xs[r * P + j], s);
                        acc[k] = s;
                    }
                }
                if (tid < C)
                    for (int r = 0; r < kRows; ++r)
                        if ((selbits >> r) & 1u) acc_b = acc_b + dzs[r * C + tid];
            }
        }
        __syncthreads();                                     // xs, zs, dzs, lse_s and tgt_s are rewritten for the next block
    }
    float *slice = a.slices + (int64_t)blockIdx.x * (CP + C + 2);
    if (grads) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int e = tid + k * kBlock;
            if (e < CP) slice[e] = acc[k];
        }
        if (tid < C) slice[CP + tid] = acc_b;
    }
    if (tid < kRows) part_s[tid] = loss_sum, corr_s[tid] = correct;
    __syncthreads();
    if (tid == 0) {
        float s = 0.0f;
        int n = 0;
        for (int r = 0; r < kRows; ++r) s = s + part_s[r], n += corr_s[r];
        slice[CP + C] = s;
        slice[CP + C + 1] = __int_as_float(n);
    }
}

// the slices added in slice order, an element per thread from e0: grad_W, grad_bias, loss = sum / M, counts
__global__ __launch_bounds__(kBlock) void node_loss_reduce_kernel(int P, int C, int S, int64_t e0, const float *__restrict__ slices,
                                                                  const int64_t *__restrict__ parts, int n_parts, float *__restrict__ grad_W,
                                                                  float *__restrict__ grad_bias, float *__restrict__ loss,
                                                                  int64_t *__restrict__ counts)
{
#pragma clang fp contract(off)
    const int64_t CP = (int64_t)C * P, stride = CP + C + 2;
    const int64_t e = e0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= stride) return;
    if (e == stride - 1) {
        if (!counts) return;
        int64_t n = 0;
        for (int b = 0; b < S; ++b) n += __float_as_int(slices[(int64_t)b * stride + e]);
        counts[0] = node_count_total(parts, n_parts), counts[1] = n;
        return;
    }
    float s = 0.0f;
    for (int b = 0; b < S; ++b) s = s + slices[(int64_t)b * stride + e];
    if (e < CP)
        grad_W[e] = s;
    else if (e < CP + C) {
        if (grad_bias) grad_bias[e - CP] = s;
    } else {
        const int64_t M = node_count_total(parts, n_parts);
        loss[0] = M > 0 ? s / (float)M : 0.0f;
    }
}

template <int NK>
int node_loss_launch(const NodeArgs &a, hipStream_t s)
{
    static sgx_lds_optin optin;                       // this instantiation's
    const int rc = sgx_raise_dynamic_lds(&node_loss_kernel<NK>, optin, kNodeLossLdsMax);
    if (rc != SGX_OK) return rc;
    hipLaunchKernelGGL(node_loss_kernel<NK>, dim3(a.S), dim3(kBlock), node_loss_lds_bytes(a.r.P, a.r.C), s, a);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

}  // namespace

extern "C" size_t sgx_node_loss_workspace_bytes(int64_t n_rows, int P, int C)
{
    if (!node_shape_ok(n_rows, P, C)) return 0;
    const int64_t nb = row_blocks(n_rows);
    const size_t S = (size_t)(nb < kGrid ? nb : kGrid);
    return kHeader + sgx_align_up(S * ((size_t)C * P + C + 2) * sizeof(float), 256);
}

extern "C" int sgx_node_loss(int64_t n_rows, int64_t n_prefix, int P, int C, const float *H, const float *W, const float *bias,
                             const int64_t *target, const uint8_t *mask, float p_drop, uint64_t seed, uint64_t step,
                             const int64_t *step_dev, float grad_scale, float *loss, int64_t *counts, float *logits, float *grad_H,
                             float *grad_W, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_rows < 1 || n_prefix < 0 || P < 1 || C < 1) return SGX_ERR_SHAPE;
    if (!H || !W || !target || !loss) return SGX_ERR_NULL;
    const bool any = grad_H || grad_W || grad_bias, all = grad_H && grad_W && (grad_bias || !bias);
    if (any && !all) return SGX_ERR_NULL;
    if (!(p_drop >= 0.0f && p_drop < 1.0f) || !node_shape_ok(n_rows, P, C)) return SGX_ERR_UNSUPPORTED;
    const size_t need = sgx_node_loss_workspace_bytes(n_rows, P, C);
    if (!workspace || workspace_bytes < need) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256) return SGX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    NodeArgs a;
    a.r = NodeRows{n_rows, n_prefix, P, C, P | 1, H, W, bias, mask, logits};
    a.n_blocks = row_blocks(n_rows), a.S = (int)(a.n_blocks < kGrid ? a.n_blocks : kGrid);
    a.target = target, a.drop = dropout_of(p_drop);
    a.seed = seed, a.step = step, a.step_dev = step_dev, a.grad_scale = grad_scale;
    a.grad_H = any ? grad_H : nullptr;
    a.parts = (const int64_t *)workspace;
    a.slices = (float *)((char *)workspace + kHeader);
    const int64_t n_sel = n_prefix < n_rows ? n_prefix : n_rows;
    const int64_t per_wg = (int64_t)kBlock * kCountPerThread;
    const int64_t count_grid = mask ? (n_sel + per_wg - 1) / per_wg : 1;
    a.n_parts = (int)(count_grid < 1 ? 1 : count_grid > kCountGrid ? kCountGrid : count_grid);
    hipLaunchKernelGGL(node_count_kernel, dim3(a.n_parts), dim3(kBlock), 0, s, n_sel, mask, (int64_t *)workspace);
    SGX_LAUNCH_CHECK();
    const int nk = (C * P + kBlock - 1) / kBlock;
    const int st = nk <= 1 ? node_loss_launch<1>(a, s) : nk <= 4 ? node_loss_launch<4>(a, s) : nk <= 16 ? node_loss_launch<16>(a, s)
                                                                                              : node_loss_launch<kAcc>(a, s);
    if (st != SGX_OK) return st;
    const int64_t stride = (int64_t)C * P + C + 2, e0 = any ? 0 : stride - 2;
    hipLaunchKernelGGL(node_loss_reduce_kernel, dim3((unsigned)((stride - e0 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, P, C, a.S, e0,
                       (const float *)a.slices, a.parts, a.n_parts, grad_W, bias ? grad_bias : nullptr, loss, counts);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
