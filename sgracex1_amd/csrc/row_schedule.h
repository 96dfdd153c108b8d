// The row schedule of a sgx_plan, stated once for the three kernels that walk it in one grid: spmm_body (spmm_csr.hip),
// gat_weighted_kernel (gat_weighted.hip) and gat_fused_kernel (gat_fused.hip).  Included at the end of sgx_device.h.
//   1. workgroups [0, split_blocks): the long rows' tasks, a wavefront per task with all its lane groups on the one row,
//      fp32 partial rows that a finalize kernel adds in task order;
//   2. workgroups [split_blocks, short_first): the rows of two steps and more, a group of LPR lanes per row, grid-strided
//      over row_order[0, n_multi) -- over all n_work rows when the tail is not taken;
//   3. workgroups from short_first on: the degree order's tail of one-step rows (at most 8 entries), 64 per wavefront, so
//      that row id -> row pointers -> entries is one round trip each for 64 rows instead of one per 64 / LPR rows.
// The host half sizes that grid, the device half tells a workgroup its part.  The inner gather loops are each kernel's own,
// and gat_weighted_kernel keeps its own text of the device half as well (measured: the comment at its head).
#pragma once

#ifndef SGX_SPMM_BLOCKS_PER_CU
#define SGX_SPMM_BLOCKS_PER_CU 512   // cap of the grid's row part (2.18 vs 2.21 ms at 64 on S-100M); rows beyond it are grid-strided
#endif

struct sgx_row_schedule {
    const int32_t *order;                  // the plan's degree order (null: natural order) and the rows it lists
    int n_work, long_threshold;            // (0: the plan has no long rows)
    int n_tasks;
    const int32_t *task_e0, *task_e1;      // (null without tasks)
    int split_blocks, n_multi, row_blocks, short_blocks, short_first;
    unsigned grid;
    bool short_tail;
};

// plan: may be null (natural order, no tasks).  lpr lanes walk a row, pass_cols = lpr x the columns of a lane = what one
// pass over the row covers.  tail_ok: what the caller's kernel asks of the tail beyond the rules here.
static inline sgx_row_schedule sgx_schedule_rows(const sgx_plan *p, int n_rows, int lpr, int pass_cols, int n_feat, bool tail_ok)
{
    constexpr int kWaves = kBlock / 64;
    sgx_row_schedule s{};
    s.order = p ? p->row_order : nullptr;
    s.n_work = s.order ? p->n_ordered : n_rows;
    s.long_threshold = (p && p->n_long > 0) ? p->long_threshold : 0;
    s.n_tasks = s.long_threshold > 0 ? p->n_tasks : 0;
    if (s.n_tasks) { s.task_e0 = p->task_e0; s.task_e1 = p->task_e1; }
    s.split_blocks = (s.n_tasks + kWaves - 1) / kWaves;
    // The tail is taken when a row's 8 entry slots are loaded by 8 lanes of its group (lpr >= 8), the plan has a degree
    // order that ends in one-step rows, one pass covers the row (the tail makes one), SGX_SPMM_NO_SHORT_TAIL is not set,
    // and the tail is worth its own workgroups: 4096 rows = 16 of them.
    s.short_tail = tail_ok && lpr >= 8 && s.order && !sgx_tune().spmm_no_short_tail && p->n_multi >= 0 && p->n_multi < s.n_work &&
                   n_feat <= pass_cols && s.n_work - p->n_multi >= 4096;
    s.n_multi = s.short_tail ? p->n_multi : s.n_work;
    s.short_blocks = s.short_tail ? (int)(((int64_t)(s.n_work - s.n_multi) + 64 * kWaves - 1) / (64 * kWaves)) : 0;
    // a ceiling, so one row block at least when there are rows and none when there are none; grid-strided past the cap
    const int64_t rows_per_block = (int64_t)(64 / lpr) * kWaves;
    int64_t row_blocks = ((int64_t)s.n_multi + rows_per_block - 1) / rows_per_block;
    if (row_blocks > 256 * SGX_SPMM_BLOCKS_PER_CU) row_blocks = 256 * SGX_SPMM_BLOCKS_PER_CU;
    s.row_blocks = (int)row_blocks;
    s.short_first = s.split_blocks + s.row_blocks;
    s.grid = (unsigned)(s.short_first + s.short_blocks);
    return s;
}

// ---- device half ----
// A lambda handed to a helper (the row store's finish) is inlined with the helper itself -- before the optimiser runs, like
// the text it replaces -- only when its call operator says so.
#define SGX_LAMBDA_INLINE __attribute__((always_inline))

// part 1: the task of this wavefront and its entries [e0, e1); index < 0 past n_tasks
struct sgx_task { int index, e0, e1; };
__device__ __forceinline__ sgx_task schedule_task(int n_tasks, const int32_t *__restrict__ task_e0, const int32_t *__restrict__ task_e1)
{
    const int task = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (task >= n_tasks) return sgx_task{-1, 0, 0};
    return sgx_task{task, task_e0[task], task_e1[task]};
}

// part 3: lane l holds row l of this wavefront's 64 tail rows -- its id, first entry and degree (at most 8: the order's last
// buckets); past the end of the order the last row stands in with degree 0 and !valid.  false: the whole tile is past the end.
struct sgx_tail_tile { int r, e0, deg; bool valid; };
__device__ __forceinline__ bool schedule_tail_tile(int short_first, int n_multi, int n_work, const int32_t *__restrict__ row_order,
                                                   const int32_t *__restrict__ rowptr, sgx_tail_tile &t)
{
    const int64_t i0 = (int64_t)n_multi + ((int64_t)((int)blockIdx.x - short_first) * (kBlock / 64) + (threadIdx.x >> 6)) * 64;
    if (i0 >= n_work) return false;
    const int64_t idx = i0 + (threadIdx.x & 63);
    t.valid = idx < n_work;
    t.r = row_order[t.valid ? idx : (int64_t)n_work - 1];
    t.e0 = rowptr[t.r];
    t.deg = t.valid ? rowptr[t.r + 1] - t.e0 : 0;
    return true;
}

// part 2: the rows of two steps and more, grid-strided over the n_walk rows ahead of the tail:
//     for (schedule_row_range<LPR, TAIL>(..., r0, step); r0 < n_walk; r0 += step) { live = schedule_row<LPR>(r0, ..., r, e0, e1); ... }
// (two functions around the kernel's own loop, not one walk that calls the kernel's body: with the body passed in as a
// functor hipcc allots registers differently in most instantiations and several lose a wavefront per SIMD,
// profiles/row_schedule_resources.md).  TAIL: the grid's row part ends at short_first, not with the grid.
template <int LPR, bool TAIL>
__device__ __forceinline__ void schedule_row_range(int split_blocks, int short_first, int64_t &first, int64_t &step)
{
    const int row_grid = (TAIL ? short_first : (int)gridDim.x) - split_blocks;
    const int64_t wave = (int64_t)(blockIdx.x - split_blocks) * (kBlock / 64) + (threadIdx.x >> 6);
    first = wave * (64 / LPR);
    step = (int64_t)row_grid * (kBlock / 64) * (64 / LPR);
}
// the row of this lane group at r0 and its entries [e0, e1).  row_order lists the rows in degree order so that the 64 / LPR
// rows of a wavefront need about the same number of steps.  false (past the end, or a long row: the tasks own it): e0 = e1.
template <int LPR>
__device__ __forceinline__ bool schedule_row(int64_t r0, int n_walk, int long_threshold, const int32_t *__restrict__ row_order,
                                             const int32_t *__restrict__ rowptr, int64_t &r, int &e0, int &e1)
{
    r = r0 + (threadIdx.x & 63) / LPR;
    e0 = e1 = 0;
    bool live = r < n_walk;
    if (live) {
        if (row_order) r = row_order[r];
        e0 = rowptr[r];
        e1 = rowptr[r + 1];
        if (long_threshold > 0 && e1 - e0 > long_threshold) live = false;
    }
    if (!live) e1 = e0;
    return live;
}

// column j of the partial rows of tasks [t0, t1) added to `start` in task order, eight loads in flight at a time (a hub row
// has tens to hundreds of tasks: one dependent load after the other was a round trip to memory each, 89 us on a 29 M-edge graph)
__device__ __forceinline__ float sum_task_partials(const float *__restrict__ partial, int ldp, int j, int t0, int t1, float start)
{
    float s = start;
    int t = t0;
    for (; t + 8 <= t1; t += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = partial[(int64_t)(t + u) * ldp + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; t < t1; ++t) s += partial[(int64_t)t * ldp + j];
    return s;
}

// A lane's VEC outputs finish(0) .. finish(VEC - 1) into columns [col0, col0 + VEC) of the row at drow: one 16-byte store
// when the chunk lies inside the row, element stores otherwise.  Which 16-byte store is the caller's:
enum sgx_row_store {
    SGX_STORE_ELEM_ALIGNED,      // through the element-aligned vector type, whatever aligned16 says (gfx950 global stores
    SGX_STORE_ELEM_ALIGNED_NT,   // need element alignment only: rows of D at P_w = 41, 47 ...); _NT: non-temporal
    SGX_STORE_ALIGNED16          // an aligned u32x4, only when aligned16
};
template <typename T, int VEC, sgx_row_store STORE, typename Finish>
__device__ __forceinline__ void store_lane_outputs(T *__restrict__ drow, int col0, int n_feat, bool aligned16, Finish &&finish)
{
    T out[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] = finish(i);
    if (VEC > 1 && (STORE != SGX_STORE_ALIGNED16 || aligned16) && col0 + VEC <= n_feat) {
        if constexpr (STORE == SGX_STORE_ALIGNED16)
            *reinterpret_cast<u32x4 *>(drow + col0) = *reinterpret_cast<const u32x4 *>(out);
        else if constexpr (STORE == SGX_STORE_ELEM_ALIGNED_NT)
            __builtin_nontemporal_store(*reinterpret_cast<const u32x4 *>(out), reinterpret_cast<typename Elem<T>::vec16_u *>(drow + col0));
        else
            *reinterpret_cast<typename Elem<T>::vec16_u *>(drow + col0) = *reinterpret_cast<const u32x4 *>(out);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (col0 + i < n_feat) drow[col0 + i] = out[i];
    }
}
