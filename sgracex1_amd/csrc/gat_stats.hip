// The GAT aggregate's row softmax statistics (sgx.h, sgx_gat_stats): per (row, head) the maximum m and the sum l of
// exp(x - m) over the row's live scores, beside the two score halves per node the aggregate's pre-pass leaves in its
// scratch.  From the four arrays any stored entry's E_e and S_e are formed again (gat_device.h, stats_weight), so a
// training forward need not write, and the backward need not read, 2 nnz heads floats.
//
// The aggregate itself is not touched: D comes from the launches sgx_gat_aggregate makes without side outputs (the one
// walk where it is taken), and one pass here forms (m, l) from the scores -- edge work only, the first stage of the
// two-stage form without its weights: per stored entry a column index, a value and a 4-byte score gather per head.
//   rows   8 lanes per row, 8 heads at a time in registers, the lanes' states merged by an xor butterfly; rows over
//          kLongRowCut entries are left to a second launch in which a workgroup looks at 8 consecutive rows and takes
//          the long ones among them with all its threads .
// Both orders are fixed, so the statistics are the same bits on every run.
#include "gat_device.h"
#include "long_rows.h"

namespace {

constexpr int kStatLanes = 8;            // lanes per row
constexpr int kStatHeads = 8;            // heads kept in registers at a time

// Both kernels keep their own text of the head-block accumulation, and the long-rows kernel its own walk over the window
// (the one long_rows.h states for gat_bwd.hip and layer_bwd.hip).  Through one accumulation function gat_row_stats_kernel
// took 62 VGPRs for 59 and row_sum of the 8-head layouts moved in its last bits (tools/gat_train_digest.py); through
// for_each_long_row the long-rows kernel took 78 VGPRs for 73 and the 8-head statistics call on the R-MAT arxiv shape went
// from 0.952 to 0.958 ms (fp32) and 0.781 to 0.787 ms (fp16), outside the parent's spread of 0.004 (profiles/long_rows_*).
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_row_stats_kernel(
    int n_rows, int n_heads, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    const float *__restrict__ s1, const float *__restrict__ s2, unsigned s2_bytes, float alpha, float *__restrict__ row_max,
    float *__restrict__ row_sum)
{
    constexpr int RPW = 64 / kStatLanes;
    const int lane = threadIdx.x & 63, sub = lane % kStatLanes, grp = lane / kStatLanes;
    const int64_t r = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * RPW + grp;
    const __amdgpu_buffer_rsrc_t s2_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(s2), 0, s2_bytes, 0x00020000);
    bool mine = r < n_rows;
    int e0 = 0, e1 = 0;
    if (mine) { e0 = rowptr[r]; e1 = rowptr[r + 1]; }
    if (e1 - e0 > kLongRowCut) { mine = false; e1 = e0; }          // the long-rows launch owns it
    for (int hb0 = 0; hb0 < n_heads; hb0 += kStatHeads) {
        float m[kStatHeads], l[kStatHeads], si[kStatHeads];
#pragma unroll
        for (int k = 0; k < kStatHeads; ++k) {
            m[k] = -INFINITY;
            l[k] = 0.0f;
            si[k] = (mine && hb0 + k < n_heads) ? s1[r * n_heads + hb0 + k] : 0.0f;
        }
        for (int idx = e0 + sub; idx < e1; idx += kStatLanes) {
            if (!(Elem<T>::to_f32(val[idx]) > 0.0f)) continue;
            const unsigned at = ((unsigned)col[idx] * (unsigned)n_heads + (unsigned)hb0) * 4u;
#pragma unroll
            for (int k = 0; k < kStatHeads; ++k)
                if (hb0 + k < n_heads) softmax_push(m[k], l[k], leaky(si[k] + buffer_f32(s2_rsrc, at + 4u * k), alpha));
        }
#pragma unroll
        for (int k = 0; k < kStatHeads; ++k) {
#pragma unroll
            for (int off = 1; off < kStatLanes; off <<= 1) softmax_merge(m[k], l[k], __shfl_xor(m[k], off), __shfl_xor(l[k], off));
            if (mine && sub == 0 && hb0 + k < n_heads) {
                const bool none = m[k] == -INFINITY;               // no live entry: the dead row's (0, 0)
                row_max[r * n_heads + hb0 + k] = none ? 0.0f : m[k];
                row_sum[r * n_heads + hb0 + k] = none ? 0.0f : l[k];
            }
        }
    }
}

// rows over kLongRowCut entries: a workgroup looks at kLongSpan consecutive rows and takes the long ones among them one after
// the other with all its threads, 8 heads at a time in registers (hub rows of a power-law graph sit next to each other:
// a span of 64 rows left one workgroup with 64 hubs in a row)
constexpr int kLongSpan = 8;
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_row_stats_long_kernel(
    int n_rows, int n_heads, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    const float *__restrict__ s1, const float *__restrict__ s2, unsigned s2_bytes, float alpha, float *__restrict__ row_max,
    float *__restrict__ row_sum)
{
    __shared__ float part_m[kBlock / 64][kStatHeads], part_l[kBlock / 64][kStatHeads];
    __shared__ unsigned long long long_mask;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r_first = (int64_t)blockIdx.x * kLongSpan;
    const __amdgpu_buffer_rsrc_t s2_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(s2), 0, s2_bytes, 0x00020000);
    if (wave == 0) {                                  // which of the rows are long: one look by the first wavefront
        const int64_t r = r_first + lane;
        const int deg = (lane < kLongSpan && r < n_rows) ? rowptr[r + 1] - rowptr[r] : 0;
        const unsigned long long mask = __ballot(deg > kLongRowCut);
        if (lane == 0) long_mask = mask;
    }
    __syncthreads();
    unsigned long long todo = long_mask;
    while (todo) {                                    // (uniform over the workgroup)
        const int64_t r = r_first + (__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        const int e0 = rowptr[r], e1 = rowptr[r + 1];
        for (int hb0 = 0; hb0 < n_heads; hb0 += kStatHeads) {
            float m[kStatHeads], l[kStatHeads], si[kStatHeads];
#pragma unroll
            for (int k = 0; k < kStatHeads; ++k) {
                m[k] = -INFINITY;
                l[k] = 0.0f;
                si[k] = hb0 + k < n_heads ? s1[r * n_heads + hb0 + k] : 0.0f;
            }
            for (int idx = e0 + (int)threadIdx.x; idx < e1; idx += kBlock) {
                if (!(Elem<T>::to_f32(val[idx]) > 0.0f)) continue;
                const unsigned at = ((unsigned)col[idx] * (unsigned)n_heads + (unsigned)hb0) * 4u;
#pragma unroll
                for (int k = 0; k < kStatHeads; ++k)
                    if (hb0 + k < n_heads) softmax_push(m[k], l[k], leaky(si[k] + buffer_f32(s2_rsrc, at + 4u * k), alpha));
            }
            __syncthreads();                          // the partial states of the previous block of heads have been read
#pragma unroll
            for (int k = 0; k < kStatHeads; ++k) {
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) softmax_merge(m[k], l[k], __shfl_xor(m[k], off), __shfl_xor(l[k], off));
                if (lane == 0) { part_m[wave][k] = m[k]; part_l[wave][k] = l[k]; }
            }
            __syncthreads();
            if (threadIdx.x < kStatHeads && hb0 + (int)threadIdx.x < n_heads) {
                const int k = threadIdx.x;
                float mm = part_m[0][k], ll = part_l[0][k];
                for (int i = 1; i < kBlock / 64; ++i) softmax_merge(mm, ll, part_m[i][k], part_l[i][k]);
                const bool none = mm == -INFINITY;
                row_max[r * n_heads + hb0 + k] = none ? 0.0f : mm;
                row_sum[r * n_heads + hb0 + k] = none ? 0.0f : ll;
            }
        }
    }
}

// E and S of every stored entry from the statistics: entry-parallel, the row of an entry by bisection of rowPtr (the
// probes of neighbouring entries coincide); the entry count is read on the device
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_edge_outputs_kernel(
    int n_rows, int n_heads, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    const float *__restrict__ score_row, const float *__restrict__ score_col, unsigned sc_bytes,
    const float *__restrict__ row_max, const float *__restrict__ row_sum, float alpha, float dead_weight,
    float *__restrict__ E, float *__restrict__ S)
{
    const __amdgpu_buffer_rsrc_t sc_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(score_col), 0, sc_bytes, 0x00020000);
    const int64_t nnz = rowptr[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock) {
        int lo = 0, hi = n_rows;                      // the last r with rowptr[r] <= e
        while (hi - lo > 1) {
            const int mid = (int)(((int64_t)lo + hi) >> 1);
            if ((int64_t)rowptr[mid] <= e) lo = mid;
            else hi = mid;
        }
        const bool live = Elem<T>::to_f32(val[e]) > 0.0f;
        const unsigned at = (unsigned)col[e] * (unsigned)n_heads * 4u;
        for (int h = 0; h < n_heads; ++h) {
            const int64_t rh = (int64_t)lo * n_heads + h;
            const float x = leaky(score_row[rh] + buffer_f32(sc_rsrc, at + 4u * h), alpha);
            if (E) E[e * n_heads + h] = x;
            if (S) S[e * n_heads + h] = stats_weight(x, live, row_max[rh], row_sum[rh], dead_weight);
        }
    }
}

}  // namespace

int sgx_gat_stats_check(const sgx_gat_stats *st, int n_cols, int n_heads)
{
    if (!st || !st->score_row || !st->score_col || !st->row_max || !st->row_sum) return SGX_ERR_NULL;
    if ((unsigned long long)n_cols * (unsigned long long)(n_heads < 1 ? 1 : n_heads) * 4ull >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;
    return SGX_OK;
}

// the statistics of an aggregate that has just run on `s_scratch`, laid out as `lay` (its scores: s1, s2 [n_cols][n_heads])
int sgx_gat_row_stats(int dtype, int n_rows, int n_cols, int n_heads, float alpha, const int32_t *rowPtr,
                      const int32_t *columnIndex, const void *values, const float *s_scratch, const sgx_gat_scratch &lay,
                      const sgx_gat_stats *st, hipStream_t stream)
{
    if (n_heads < 1) n_heads = 1;
    if (n_rows <= 0) return SGX_OK;
    const float *s1 = s_scratch + lay.s1, *s2 = s_scratch + lay.s2;
    SGX_HIP_CHECK(hipMemcpyAsync(st->score_row, s1, (size_t)n_rows * n_heads * sizeof(float), hipMemcpyDeviceToDevice, stream));
    SGX_HIP_CHECK(hipMemcpyAsync(st->score_col, s2, (size_t)n_cols * n_heads * sizeof(float), hipMemcpyDeviceToDevice, stream));
    const unsigned s2_bytes = (unsigned)((size_t)n_cols * n_heads * 4);
    const int rows_per_block = (64 / kStatLanes) * (kBlock / 64);
    const dim3 grid((unsigned)((n_rows + rows_per_block - 1) / rows_per_block)), grid_long((unsigned)((n_rows + kLongSpan - 1) / kLongSpan));
    return sgx_dtype_dispatch(dtype, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL(gat_row_stats_kernel<T>, grid, dim3(kBlock), 0, stream, n_rows, n_heads, rowPtr, columnIndex,
                           (const T *)values, s1, s2, s2_bytes, alpha, st->row_max, st->row_sum);
        SGX_LAUNCH_CHECK();
        hipLaunchKernelGGL(gat_row_stats_long_kernel<T>, grid_long, dim3(kBlock), 0, stream, n_rows, n_heads, rowPtr, columnIndex,
                           (const T *)values, s1, s2, s2_bytes, alpha, st->row_max, st->row_sum);
        SGX_LAUNCH_CHECK();
        return SGX_OK;
    });
}

extern "C" int sgx_gat_aggregate_stats(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha,
                                       const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                       const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd,
                                       const float *fill, int64_t n_nodes, const sgx_plan *plan, float *s_scratch,
                                       const sgx_gat_stats *stats, void *stream)
{
    if (n_heads < 1) n_heads = 1;
    int fill_dead_rows = 0;
    if (fill) {
        if (n_nodes < 1 || n_nodes > 0x7FFFFFFF) return SGX_ERR_SHAPE;
    } else if (n_nodes != 0) {
        if (n_nodes != n_cols) return SGX_ERR_SHAPE;
        fill_dead_rows = 1;
    }
    if (n_cols >= 0) {
        const int rc = sgx_gat_stats_check(stats, n_cols, n_heads);
        if (rc != SGX_OK) return rc;
    }
    const int rc = sgx_gat_aggregate_ep(dtype, relu, fill_dead_rows, n_rows, n_cols, n_feat, n_heads, alpha, rowPtr, columnIndex,
                                        values, Wh, ldh, attention, D, ldd, nullptr, nullptr, plan, s_scratch, (hipStream_t)stream,
                                        0.0f, fill, (int)n_nodes);
    if (rc != SGX_OK) return rc;
    return sgx_gat_row_stats(dtype, n_rows, n_cols, n_heads, alpha, rowPtr, columnIndex, values, s_scratch,
                             sgx_gat_scratch_layout(n_cols, n_feat, n_heads, fill_dead_rows, plan), stats, (hipStream_t)stream);
}

extern "C" int sgx_gat_edge_outputs(int dtype_values, int n_rows, int n_cols, int n_heads, float alpha,
                                    const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                    const sgx_gat_stats *stats, float dead_weight, float *E, float *S, void *stream)
{
    if (n_heads < 1) n_heads = 1;
    if (n_rows < 0 || n_cols < 0) return SGX_ERR_SHAPE;
    if (n_rows == 0 || (!E && !S)) return SGX_OK;
    if (!rowPtr || !columnIndex || !values) return SGX_ERR_NULL;
    const int rc = sgx_gat_stats_check(stats, n_cols, n_heads);
    if (rc != SGX_OK) return rc;
    if (dtype_values != SGX_F16 && dtype_values != SGX_F32) return SGX_ERR_UNSUPPORTED;
    const unsigned sc_bytes = (unsigned)((size_t)n_cols * n_heads * 4);
    const dim3 grid((unsigned)sgx_cu_count(1) * 8u);               // persistent: 8 workgroups per CU
    return sgx_dtype_dispatch(dtype_values, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL(gat_edge_outputs_kernel<T>, grid, dim3(kBlock), 0, (hipStream_t)stream, n_rows, n_heads, rowPtr,
                           columnIndex, (const T *)values, stats->score_row, stats->score_col, sc_bytes, stats->row_max,
                           stats->row_sum, alpha, dead_weight, E, S);
        SGX_LAUNCH_CHECK();
        return SGX_OK;
    });
}
