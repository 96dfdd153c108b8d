// The layer's backward as one call (sgx_layer_backward, sgx.h): what FPYNQ_GAT.backward composes from stage calls and
// torch glue, run on the same stage kernels with the same arguments, plus three kernels of its own:
//
//   attention gradient   [Wh^T g1 ; Wh^T colsum(sg)] without a transposed pattern.  Wh^T colsum(sg) = sum_e sg_e Wh[col_e]
//                        is a gather over the stored entries in ROW order -- the aggregation's access pattern:
//                            t_r[f] = sum_{e in r} sg_e Wh[col_e][f]          an fp32 fma chain in CSR order from 0
//                        LPR lanes (16 bytes of the row each) form t_r of one row, 64 / LPR rows to a wavefront; a
//                        workgroup owns a run of consecutive rows, every lane group walks its share of them in ascending
//                        order and adds t_r and g1[r] Wh[r] into registers; the lane groups' sums are added in a fixed
//                        order through LDS into the workgroup's slice of the workspace (plain stores, no atomics) and a
//                        second launch adds the slices in slice order.  A row over 256 entries is left out of that walk
//                        and taken by the whole workgroup afterwards (long_rows.h): chunks of 256 entries, one per lane
//                        group, their partial sums added in chunk order.  The grid depends on the shapes only.
//   dead-row select      pg[r][:] = colsum(G)[:] * (1 / N) where dead[r], in place (the torch.where of the Python path):
//                        a wavefront per row, rows by grid stride.
//   casts                fp16 -> fp32 of the GCN adjacency values (and of a dense fp16 X for Wh = X . W).
#include "gat_device.h"
#include "long_rows.h"

namespace {

constexpr int kAgChunk = kLongRowCut;    // entries of a long row one lane group takes at a time: the cut is the chunk
constexpr int kAgRowsPerSlice = 64;      // a slice per this many rows ...
constexpr int kAgMaxSlices = 1024;       // ... up to this many slices

static inline int ag_slices(int n_rows)
{
    int s = (n_rows + kAgRowsPerSlice - 1) / kAgRowsPerSlice;
    if (s < 1) s = 1;
    return s > kAgMaxSlices ? kAgMaxSlices : s;
}

// 16 bytes (VEC) or four elements of row `off` of Wh at byte offset `at`; kOOB and whatever lies past the table read 0
template <bool VEC>
__device__ __forceinline__ void load_wh4(__amdgpu_buffer_rsrc_t rsrc, unsigned at, float *w)
{
    union { u32x4 v; float f[4]; } u;
    if constexpr (VEC) {
        u.v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, at, 0, 0);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) u.v[i] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, at == kOOB ? kOOB : at + 4u * i, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = u.f[i];
}

// t[0..3] += sum over entries [e0, e1) of sg_e Wh[col_e][col0 .. col0 + 3], one fma per entry and column, in entry order
template <bool VEC>
__device__ __forceinline__ void gather_chain(__amdgpu_buffer_rsrc_t w_rsrc, const int32_t *__restrict__ col, const float *__restrict__ sg,
                                             int e0, int e1, unsigned ldw_bytes, int col0, bool col_in, float *t)
{
    for (int e = e0; e < e1; e += 4) {
        float s[4], w[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                           // four rows in flight, added in order below
            const bool have = e + j < e1;
            const int c = have ? col[e + j] : 0;
            s[j] = have ? sg[e + j] : 0.0f;
            load_wh4<VEC>(w_rsrc, (have && col_in) ? (unsigned)c * ldw_bytes + (unsigned)col0 * 4u : kOOB, w[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < e1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = __builtin_fmaf(s[j], w[j][i], t[i]);
            }
    }
}

template <int LPR, bool VEC>
__global__ __launch_bounds__(kBlock) void attention_grad_slices_kernel(
    int n_rows, int n_feat, int rows_per_slice, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ sg, const float *__restrict__ g1, const float *__restrict__ Wh, unsigned w_bytes, unsigned ldw_bytes,
    float *__restrict__ slices)
{
    constexpr int GROUPS = 64 / LPR;               // rows a wavefront works on at a time
    constexpr int TILE = LPR * 4;                  // columns a lane group covers per pass
    constexpr int WAVES = kBlock / 64;
    constexpr int WORKERS = WAVES * GROUPS;        // lane groups of the workgroup
    __shared__ float part[WORKERS * TILE];         // 1024 floats whatever LPR
    __shared__ unsigned long long long_mask;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane % LPR, grp = lane / LPR;
    const int worker = wave * GROUPS + grp;
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wh), 0, w_bytes, 0x00020000);
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_slice;
    const int64_t r1 = r0 + rows_per_slice < n_rows ? r0 + rows_per_slice : n_rows;
    float *__restrict__ slice = slices + (size_t)blockIdx.x * 2u * (size_t)n_feat;

    // the workgroup's partial sums of one column tile, added worker by worker in worker order by the tile's first threads
    auto fold = [&](const float *v) -> float {
        __syncthreads();                                   // the previous use of `part` has been read
#pragma unroll
        for (int i = 0; i < 4; ++i) part[worker * TILE + sub * 4 + i] = v[i];
        __syncthreads();
        float t = 0.0f;
        if ((int)threadIdx.x < TILE)
            for (int k = 0; k < WORKERS; ++k) t += part[k * TILE + threadIdx.x];
        return t;
    };

    for (int c0 = 0; c0 < n_feat; c0 += TILE) {
        const int col0 = c0 + sub * 4;
        const bool col_in = col0 < n_feat;
        float a1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        // rows of up to kAgChunk entries: one lane group each, ascending
        for (int64_t r = r0 + worker; r < r1; r += WORKERS) {
            const int e0 = rowptr[r], e1 = rowptr[r + 1];
            float w[4];
            load_wh4<VEC>(w_rsrc, col_in ? (unsigned)r * ldw_bytes + (unsigned)col0 * 4u : kOOB, w);
            const float g = g1[r];
#pragma unroll
            for (int i = 0; i < 4; ++i) a1[i] = __builtin_fmaf(g, w[i], a1[i]);
            if (e1 - e0 <= kAgChunk) {
                float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                gather_chain<VEC>(w_rsrc, col, sg, e0, e1, ldw_bytes, col0, col_in, t);
#pragma unroll
                for (int i = 0; i < 4; ++i) a2[i] += t[i];
            }
        }
        const float s1 = fold(a1);
        float s2 = fold(a2);
        // longer rows, in ascending order: the whole workgroup, a chunk per lane group, chunk sums added in chunk order
        for (int64_t win = r0; win < r1; win += 64)
            for_each_long_row<64, kAgChunk>(rowptr, win, r1, &long_mask, [&](int64_t r) SGX_LAMBDA_INLINE {
                const int e0 = rowptr[r], e1 = rowptr[r + 1];
                const int n_chunks = (e1 - e0 + kAgChunk - 1) / kAgChunk;
                float row_t = 0.0f;
                for (int cb = 0; cb < n_chunks; cb += WORKERS) {
                    float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    const int k = cb + worker;
                    if (k < n_chunks) {
                        const int c_e0 = e0 + k * kAgChunk;
                        const int c_e1 = c_e0 + kAgChunk < e1 ? c_e0 + kAgChunk : e1;
                        gather_chain<VEC>(w_rsrc, col, sg, c_e0, c_e1, ldw_bytes, col0, col_in, t);
                    }
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < 4; ++i) part[worker * TILE + sub * 4 + i] = t[i];
                    __syncthreads();
                    const int n_here = n_chunks - cb < WORKERS ? n_chunks - cb : WORKERS;
                    if ((int)threadIdx.x < TILE)
                        for (int j = 0; j < n_here; ++j) row_t += part[j * TILE + threadIdx.x];
                }
                s2 += row_t;
            });
        if ((int)threadIdx.x < TILE && c0 + (int)threadIdx.x < n_feat) {
            slice[c0 + threadIdx.x] = s1;
            slice[n_feat + c0 + threadIdx.x] = s2;
        }
    }
}

// out[j] = the slices' entries j added in slice order
__global__ __launch_bounds__(kBlock) void attention_grad_reduce_kernel(int n_slices, int width, const float *__restrict__ slices,
                                                                       float *__restrict__ out)
{
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < width; j += (int64_t)gridDim.x * kBlock) {
        float t = 0.0f;
        for (int s = 0; s < n_slices; ++s) t += slices[(size_t)s * width + j];
        out[j] = t;
    }
}

// pg[r][c] = sums[c] * inv_n for the rows with dead[r]: a wavefront per row, which leaves at once unless the row is dead
__global__ __launch_bounds__(kBlock) void dead_row_select_kernel(int n_rows, int n_feat, const uint8_t *__restrict__ dead,
                                                                 const float *__restrict__ sums, float inv_n, float *__restrict__ pg,
                                                                 int64_t ldp)
{
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); r < n_rows; r += (int64_t)gridDim.x * (kBlock / 64)) {
        if (!dead[r]) continue;
        for (int c = lane; c < n_feat; c += 64) pg[r * ldp + c] = sums[c] * inv_n;
    }
}

// out[i] = in[i] * f
__global__ __launch_bounds__(kBlock) void scale_kernel(int n, const float *__restrict__ in, float f, float *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) out[i] = in[i] * f;
}

// out[r] = in[r * ld]
__global__ __launch_bounds__(kBlock) void first_column_kernel(int n, const float *__restrict__ in, int64_t ld, float *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) out[i] = in[i * ld];
}

// out[r][c] = (float)in[r][c]
__global__ __launch_bounds__(kBlock) void cast_f16_f32_kernel(int64_t n_rows, int n_cols, const f16 *__restrict__ in, int64_t ldi,
                                                              float *__restrict__ out, int64_t ldo)
{
    const int64_t total = n_rows * n_cols;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
        const int64_t r = idx / n_cols;
        const int c = (int)(idx - r * n_cols);
        out[r * ldo + c] = (float)in[r * ldi + c];
    }
}

// workgroups for n items, one per thread, capped: every kernel launched with it walks its items by grid stride
static inline unsigned blocks_for(int64_t n)
{
    int64_t b = (n + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    return (unsigned)(b > 65536 ? 65536 : b);
}

int cast_f16_f32(int64_t n_rows, int n_cols, const void *in, int64_t ldi, float *out, int64_t ldo, hipStream_t s)
{
    if (n_rows <= 0 || n_cols <= 0) return SGX_OK;
    hipLaunchKernelGGL(cast_f16_f32_kernel, dim3(blocks_for(n_rows * n_cols)), dim3(kBlock), 0, s, n_rows, n_cols, (const f16 *)in, ldi,
                       out, ldo);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

template <int LPR>
int ag_launch(bool vec, unsigned grid, hipStream_t s, int n_rows, int n_feat, int rps, const int32_t *rowptr, const int32_t *col,
              const float *sg, const float *g1, const float *Wh, unsigned w_bytes, unsigned ldw_bytes, float *slices)
{
    if (vec)
        hipLaunchKernelGGL((attention_grad_slices_kernel<LPR, true>), dim3(grid), dim3(kBlock), 0, s, n_rows, n_feat, rps, rowptr, col, sg,
                           g1, Wh, w_bytes, ldw_bytes, slices);
    else
        hipLaunchKernelGGL((attention_grad_slices_kernel<LPR, false>), dim3(grid), dim3(kBlock), 0, s, n_rows, n_feat, rps, rowptr, col, sg,
                           g1, Wh, w_bytes, ldw_bytes, slices);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

// workspace of the layer's backward, byte offsets (all multiples of 256)
struct Carve {
    size_t adj32, x32, wt, wh, sg, g1, s_out, cs, cs_scratch, mean, drs_tmp, drs, pg, ag, spmm, xtg, total;
    int64_t ldwh;
    // behind the layout above: the scratch of the entry-split calls, with its size
    size_t flat_adj, flat_adj_bytes, flat_ag, flat_ag_bytes, flat_fea, flat_fea_bytes, flat_xt, flat_xt_bytes;
};

// which of the three schedule fields the call reads, and takes as SGX_SCHEDULE_FLAT
static inline bool reads_fea(const sgx_layer_grad_desc *d) { return d->gat_mode == 1 && d->gemm_mode == 0; }
static inline bool reads_xt(const sgx_layer_grad_desc *d) { return d->gemm_mode == 0; }
static inline bool flat_adj(const sgx_layer_grad_desc *d) { return d->schedule_adj == SGX_SCHEDULE_FLAT; }
static inline bool flat_fea(const sgx_layer_grad_desc *d) { return reads_fea(d) && d->schedule_fea == SGX_SCHEDULE_FLAT; }
static inline bool flat_xt(const sgx_layer_grad_desc *d) { return reads_xt(d) && d->schedule_xt == SGX_SCHEDULE_FLAT; }
static inline bool schedule_known(int s) { return s == SGX_SCHEDULE_DEFAULT || s == SGX_SCHEDULE_FLAT; }

int check_desc(const sgx_layer_grad_desc *d)
{
    if (!d) return SGX_ERR_NULL;
    if (d->gat_heads > 1) return SGX_ERR_UNSUPPORTED;
    if (d->gat_mode != 0 && d->gat_mode != 1) return SGX_ERR_UNSUPPORTED;
    if (d->gemm_mode != 0 && d->gemm_mode != 1) return SGX_ERR_UNSUPPORTED;
    if (!schedule_known(d->schedule_adj) || (reads_fea(d) && !schedule_known(d->schedule_fea)) ||
        (reads_xt(d) && !schedule_known(d->schedule_xt)))
        return SGX_ERR_UNSUPPORTED;
    if ((flat_adj(d) && d->plan_adj) || (flat_fea(d) && d->plan_fea) || (flat_xt(d) && d->plan_xt)) return SGX_ERR_UNSUPPORTED;
    if (flat_adj(d) && d->nnz_adj > 0x7fffffffll) return SGX_ERR_SHAPE;
    if ((flat_fea(d) && (d->nnz_fea < 0 || d->nnz_fea > 0x7fffffffll)) || (flat_xt(d) && (d->nnz_xt < 0 || d->nnz_xt > 0x7fffffffll)))
        return SGX_ERR_SHAPE;
    if (d->N_adj < 1 || d->M_adj < 1 || d->M_fea < 1 || d->P_w < 1 || d->nnz_adj < 0) return SGX_ERR_SHAPE;
    if (d->N_adj != d->M_adj) return SGX_ERR_SHAPE;                            // P . G needs a square P
    if (!flat_adj(d) && d->nnz_adj >= 0x7fffffffll) return SGX_ERR_UNSUPPORTED;          // (a flat capacity reaches INT32_MAX, as the entry-split calls do)
    if (d->dtype_adj != SGX_F16 && d->dtype_adj != SGX_F32) return SGX_ERR_UNSUPPORTED;
    if (!d->rowPtr_adj || !d->columnIndex_adj || !d->values_adj || !d->W || !d->G || !d->grad_weights) return SGX_ERR_NULL;
    if (d->ldg < d->P_w) return SGX_ERR_SHAPE;
    if (d->grad_input && d->ld_gi < d->M_fea) return SGX_ERR_SHAPE;
    if (d->gemm_mode == 1) {
        if (d->dtype_x != SGX_F16 && d->dtype_x != SGX_F32) return SGX_ERR_UNSUPPORTED;
        if (!d->X) return SGX_ERR_NULL;
        if (d->ldx < d->M_fea) return SGX_ERR_SHAPE;
    } else {
        if (!d->rowPtr_xt || !d->columnIndex_xt || !d->values_xt) return SGX_ERR_NULL;
        if (d->gat_mode && (!d->rowPtr_fea || !d->columnIndex_fea || !d->values_fea)) return SGX_ERR_NULL;
    }
    if (d->gat_mode) {
        if (!d->grad_attention) return SGX_ERR_NULL;
        const bool es = d->E || d->S;
        if (es && d->stats) return SGX_ERR_UNSUPPORTED;                        // one form of the forward's state, not both
        if (!es && !d->stats) return SGX_ERR_NULL;
        if (es && (!d->E || !d->S)) return SGX_ERR_NULL;
        if (d->stats) {
            const int rc = sgx_gat_stats_check(d->stats, d->M_adj, 1);
            if (rc != SGX_OK) return rc;
        }
        const unsigned long long w_bytes = (unsigned long long)d->M_adj * (unsigned long long)sgx_ldh(SGX_F32, d->P_w) * 4ull;
        const unsigned long long g_bytes = (unsigned long long)d->N_adj * (unsigned long long)d->ldg * 4ull;
        if (w_bytes >= 0xFFFFFFF0ull || g_bytes >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;   // the edge pass's 32-bit offsets
    }
    // the entry-split calls take tables inside 32-bit byte offsets only: G (P . G), W (X . W), pg (X^T . pg)
    if ((flat_adj(d) && sgx_spmm_table_big(SGX_F32, d->M_adj, d->ldg, d->P_w)) ||
        (flat_fea(d) && sgx_spmm_table_big(SGX_F32, d->M_fea, d->P_w, d->P_w)) ||
        (flat_xt(d) && sgx_spmm_table_big(SGX_F32, d->N_adj, d->P_w, d->P_w)))
        return SGX_ERR_UNSUPPORTED;
    if (flat_adj(d) && (unsigned long long)d->ldg * 4ull >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;
    return SGX_OK;
}

Carve carve(const sgx_layer_grad_desc *d)
{
    Carve c{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += sgx_align_up(bytes, 256); return here; };
    const size_t n = (size_t)d->N_adj, P = (size_t)d->P_w, M = (size_t)d->M_fea, nnz = (size_t)d->nnz_adj;
    const size_t cs_bytes = sgx_col_sums_scratch_bytes(d->P_w);
    c.ldwh = sgx_ldh(SGX_F32, d->P_w);
    c.adj32 = (!d->gat_mode && d->dtype_adj == SGX_F16) ? take((nnz + 1) * 4) : 0;
    c.cs = take(P * 4);
    c.cs_scratch = take(cs_bytes);
    c.pg = take(n * P * 4);
    if (d->gat_mode) {
        c.x32 = (d->gemm_mode == 1 && d->dtype_x == SGX_F16) ? take(n * M * 4) : 0;
        c.wt = d->gemm_mode == 1 ? take(P * M * 4) : 0;
        c.wh = take(n * (size_t)c.ldwh * 4);
        c.sg = take((nnz + 1) * 4);
        c.g1 = take(n * 4);
        c.s_out = d->stats ? take((nnz + 1) * 4) : 0;
        c.mean = take(P * 4);
        c.drs_tmp = take(n * 4 * 4);
        c.drs = take(n * 4);
        c.ag = take((size_t)ag_slices(d->N_adj) * 2 * P * 4);
    }
    size_t spmm = sgx_spmm_scratch_bytes(d->plan_adj, d->P_w);
    if (d->gemm_mode == 0) {
        const size_t a = sgx_spmm_scratch_bytes(d->plan_xt, d->P_w), b = d->gat_mode ? sgx_spmm_scratch_bytes(d->plan_fea, d->P_w) : 0;
        spmm = spmm > a ? spmm : a;
        spmm = spmm > b ? spmm : b;
    }
    c.spmm = take(spmm);
    c.xtg = d->gemm_mode == 1 ? take(sgx_xt_g_workspace_bytes(d->N_adj, d->M_fea, d->P_w)) : 0;
    auto take_sized = [&](bool wanted, size_t bytes, size_t &size) { size = wanted ? bytes : 0; return wanted ? take(bytes) : (size_t)0; };
    c.flat_adj = take_sized(flat_adj(d), sgx_spmm_flat_scratch_bytes(d->nnz_adj, d->P_w), c.flat_adj_bytes);
    c.flat_ag = take_sized(flat_adj(d) && d->gat_mode, sgx_gat_attention_grad_flat_workspace_bytes(d->nnz_adj, d->N_adj, d->P_w),
                           c.flat_ag_bytes);
    c.flat_fea = take_sized(flat_fea(d), sgx_spmm_flat_scratch_bytes(d->nnz_fea, d->P_w), c.flat_fea_bytes);
    c.flat_xt = take_sized(flat_xt(d), sgx_spmm_flat_scratch_bytes(d->nnz_xt, d->P_w), c.flat_xt_bytes);
    c.total = at;
    return c;
}

}  // namespace

extern "C" int sgx_gat_attention_grad(int n_rows, int n_cols, int n_feat, const int32_t *rowPtr, const int32_t *columnIndex,
                                      const float *sg, const float *g1, const float *Wh, int64_t ldw, float *grad_attention,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_rows < 0 || n_cols < n_rows || n_feat < 1 || ldw < n_feat) return SGX_ERR_SHAPE;
    if (!grad_attention) return SGX_ERR_NULL;
    if (n_rows > 0 && (!rowPtr || !columnIndex || !sg || !g1 || !Wh)) return SGX_ERR_NULL;
    const unsigned long long w_bytes = (unsigned long long)n_cols * (unsigned long long)ldw * 4ull;
    if (w_bytes >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;
    const int n_slices = ag_slices(n_rows);
    if (!workspace || workspace_bytes < (size_t)n_slices * 2 * (size_t)n_feat * 4) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256 != 0) return SGX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int rps = n_rows > 0 ? (n_rows + n_slices - 1) / n_slices : 1;
    const bool vec = (uintptr_t)Wh % 16 == 0 && (ldw * 4) % 16 == 0;
    int lpr = sgx_next_pow2((n_feat + 3) / 4);
    if (lpr > 64) lpr = 64;
    float *slices = (float *)workspace;
    int rc;
#define SGX_AG(L) rc = ag_launch<L>(vec, (unsigned)n_slices, s, n_rows, n_feat, rps, rowPtr, columnIndex, sg, g1, Wh, (unsigned)w_bytes, \
                                    (unsigned)(ldw * 4), slices)
    switch (lpr) {
    case 1: SGX_AG(1); break;
    case 2: SGX_AG(2); break;
    case 4: SGX_AG(4); break;
    case 8: SGX_AG(8); break;
    case 16: SGX_AG(16); break;
    case 32: SGX_AG(32); break;
    default: SGX_AG(64); break;
    }
#undef SGX_AG
    if (rc != SGX_OK) return rc;
    hipLaunchKernelGGL(attention_grad_reduce_kernel, dim3(blocks_for(2 * (int64_t)n_feat)), dim3(kBlock), 0, s, n_slices, 2 * n_feat, slices,
                       grad_attention);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

extern "C" size_t sgx_gat_attention_grad_workspace_bytes(int n_rows, int n_feat)
{
    if (n_rows < 0 || n_feat < 1) return 0;
    return sgx_align_up((size_t)ag_slices(n_rows) * 2 * (size_t)n_feat * 4, 256);
}

extern "C" size_t sgx_layer_backward_workspace_bytes(const sgx_layer_grad_desc *d)
{
    if (check_desc(d) != SGX_OK) return 0;
    return carve(d).total;
}

extern "C" int sgx_layer_backward_schedule(const sgx_layer_grad_desc *d)
{
    const int rc = check_desc(d);
    if (rc != SGX_OK) return rc;
    return (flat_adj(d) ? 1 : 0) | (flat_fea(d) ? 2 : 0) | (flat_xt(d) ? 4 : 0);
}

extern "C" int sgx_layer_backward(const sgx_layer_grad_desc *d, void *stream)
{
    int rc = check_desc(d);
    if (rc != SGX_OK) return rc;
    const Carve c = carve(d);
    if (!d->workspace || d->workspace_bytes < c.total) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)d->workspace % 256 != 0) return SGX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)d->workspace;
    const int n = d->N_adj, P = d->P_w, M = d->M_fea;
    const float inv_n = 1.0f / (float)d->M_adj;
    float *cs = (float *)(ws + c.cs), *cs_scratch = (float *)(ws + c.cs_scratch), *pg = (float *)(ws + c.pg);
    void *spmm_scratch = ws + c.spmm;
    const float *p_values;

    if (d->gat_mode) {
        float *Wh = (float *)(ws + c.wh), *sg = (float *)(ws + c.sg), *g1 = (float *)(ws + c.g1);
        // Wh = X . W, fp32
        if (d->gemm_mode == 1) {
            const void *X = d->X;
            int64_t ldx = d->ldx;
            if (d->dtype_x == SGX_F16) {
                rc = cast_f16_f32(n, M, d->X, d->ldx, (float *)(ws + c.x32), M, s);
                if (rc != SGX_OK) return rc;
                X = ws + c.x32;
                ldx = M;
            }
            float *Wt = (float *)(ws + c.wt);
            rc = sgx_transpose(SGX_F32, M, P, d->W, P, Wt, M, stream);
            if (rc != SGX_OK) return rc;
            rc = sgx_xw_dense(SGX_F32, SGX_ACC_F32, 1, n, M, P, X, ldx, Wt, M, Wh, c.ldwh, stream);
        } else if (flat_fea(d)) {                            // a CSR X . W is an aggregation over the rows of W
            rc = sgx_spmm_csr_flat(SGX_F32, 0, n, M, P, d->nnz_fea, d->rowPtr_fea, d->columnIndex_fea, d->values_fea, d->W, P, Wh, c.ldwh,
                                   ws + c.flat_fea, c.flat_fea_bytes, stream);
        } else {
            rc = sgx_xw_sparse(SGX_F32, SGX_ACC_F32, 1, n, M, P, d->rowPtr_fea, d->columnIndex_fea, d->values_fea, d->W, P, Wh, c.ldwh,
                               d->plan_fea, spmm_scratch, sgx_spmm_scratch_bytes(d->plan_fea, P), stream);
        }
        if (rc != SGX_OK) return rc;
        // the softmax row sum of a dead row: G[r] . colsum(Wh) / N
        float *drs = nullptr;
        if (d->dead) {
            float *mean = (float *)(ws + c.mean), *tmp = (float *)(ws + c.drs_tmp);
            drs = (float *)(ws + c.drs);
            rc = sgx_col_sums(SGX_F32, n, P, Wh, c.ldwh, cs, cs_scratch, stream);
            if (rc != SGX_OK) return rc;
            hipLaunchKernelGGL(scale_kernel, dim3(blocks_for(P)), dim3(kBlock), 0, s, P, cs, inv_n, mean);
            SGX_LAUNCH_CHECK();
            rc = sgx_xw_dense(SGX_F32, SGX_ACC_F32, 1, n, P, 1, d->G, d->ldg, mean, P, tmp, 4, stream);
            if (rc != SGX_OK) return rc;
            hipLaunchKernelGGL(first_column_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, n, tmp, (int64_t)4, drs);
            SGX_LAUNCH_CHECK();
        }
        if (d->stats) {
            float *S_out = (float *)(ws + c.s_out);
            rc = sgx_gat_backward_edges_stats(d->dtype_adj, n, d->M_adj, P, 1, d->alpha, d->rowPtr_adj, d->columnIndex_adj, d->values_adj,
                                              d->stats, d->dead_weight, d->G, d->ldg, Wh, c.ldwh, d->dead, drs, sg, g1, S_out, stream);
            p_values = S_out;
        } else {
            rc = sgx_gat_backward_edges(d->dtype_adj, n, d->M_adj, P, d->alpha, d->rowPtr_adj, d->columnIndex_adj, d->values_adj, d->E,
                                        d->S, d->G, d->ldg, Wh, c.ldwh, d->dead, drs, sg, g1, stream);
            p_values = d->S;
        }
        if (rc != SGX_OK) return rc;
        if (flat_adj(d))
            rc = sgx_gat_attention_grad_flat(n, d->M_adj, P, d->nnz_adj, d->rowPtr_adj, d->columnIndex_adj, sg, g1, Wh, c.ldwh,
                                             d->grad_attention, ws + c.flat_ag, c.flat_ag_bytes, stream);
        else
            rc = sgx_gat_attention_grad(n, d->M_adj, P, d->rowPtr_adj, d->columnIndex_adj, sg, g1, Wh, c.ldwh, d->grad_attention, ws + c.ag,
                                        (size_t)ag_slices(n) * 2 * (size_t)P * 4, stream);
        if (rc != SGX_OK) return rc;
    } else if (d->dtype_adj == SGX_F16) {
        rc = cast_f16_f32(1, (int)d->nnz_adj, d->values_adj, d->nnz_adj, (float *)(ws + c.adj32), d->nnz_adj, s);
        if (rc != SGX_OK) return rc;
        p_values = (const float *)(ws + c.adj32);
    } else {
        p_values = (const float *)d->values_adj;
    }

    // pg = P . G
    if (flat_adj(d))
        rc = sgx_spmm_csr_flat(SGX_F32, 0, n, d->M_adj, P, d->nnz_adj, d->rowPtr_adj, d->columnIndex_adj, p_values, d->G, d->ldg, pg, P,
                               ws + c.flat_adj, c.flat_adj_bytes, stream);
    else
        rc = sgx_spmm_csr(SGX_F32, SGX_ACC_F32, 1, 0, n, d->M_adj, P, d->rowPtr_adj, d->columnIndex_adj, p_values, d->G, d->ldg, pg, P,
                          d->plan_adj, spmm_scratch, sgx_spmm_scratch_bytes(d->plan_adj, P), stream);
    if (rc != SGX_OK) return rc;
    if (d->gat_mode && d->dead) {                                               // a dead row of P is 1/N on every column
        rc = sgx_col_sums(SGX_F32, n, P, d->G, d->ldg, cs, cs_scratch, stream);
        if (rc != SGX_OK) return rc;
        hipLaunchKernelGGL(dead_row_select_kernel, dim3(blocks_for((int64_t)n * 64)), dim3(kBlock), 0, s, n, P, d->dead, cs, inv_n, pg,
                           (int64_t)P);
        SGX_LAUNCH_CHECK();
    }
    if (d->grad_input) {                                                         // pg . W^T
        rc = sgx_xw_dense(SGX_F32, SGX_ACC_F32, 1, n, P, M, pg, P, d->W, P, d->grad_input, d->ld_gi, stream);
        if (rc != SGX_OK) return rc;
    }
    if (d->gemm_mode == 1)                                                       // X^T . pg
        return sgx_xt_g(d->dtype_x, n, M, P, d->X, d->ldx, pg, P, d->grad_weights, P, ws + c.xtg,
                        sgx_xt_g_workspace_bytes(n, M, P), stream);
    if (flat_xt(d))
        return sgx_spmm_csr_flat(SGX_F32, 0, M, n, P, d->nnz_xt, d->rowPtr_xt, d->columnIndex_xt, d->values_xt, pg, P, d->grad_weights, P,
                                 ws + c.flat_xt, c.flat_xt_bytes, stream);
    return sgx_spmm_csr(SGX_F32, SGX_ACC_F32, 1, 0, M, n, P, d->rowPtr_xt, d->columnIndex_xt, d->values_xt, pg, P, d->grad_weights, P,
                        d->plan_xt, spmm_scratch, sgx_spmm_scratch_bytes(d->plan_xt, P), stream);
}
