// The one-pass form of the GAT aggregate (gat.hip states the arithmetic and chooses the form): the softmax runs over the
// CSR row -- one group of LPR lanes per row (the same sblock layout as spmm_csr.hip) walks the edges once with a running
// (max, sum, weighted row) state, rescaled when the maximum moves; the row is normalised at the end.  The hardware's
// per-edge side outputs E (pre-softmax) and S (softmax) (SG.py:500-502) are optional (S costs a second, gather-free walk
// over the row once its max and sum are known).  It needs no plan and no stored-entry count, so every adjacency without
// a plan runs through it; with a plan that has long rows, those go through the plan's tasks.
#include "gat_device.h"

namespace {

template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void gat_aggregate_kernel(
    int n_rows, int n_cols, int n_feat, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const T *__restrict__ val, const T *__restrict__ Wh, unsigned h_bytes, unsigned ld_bytes,
    const float *__restrict__ s1, const float *__restrict__ s2, float alpha,
    T *__restrict__ D, int64_t ldd, int relu, float *__restrict__ E, float *__restrict__ S, int vec_store,
    const float *__restrict__ fill, int long_threshold, float out_scale)
{
    constexpr int RPW = 64 / LPR;
    constexpr int TILE = LPR * VEC;
    constexpr int UNR = LPR < 8 ? LPR : 8;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const int64_t r = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * RPW + grp;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Wh), 0, h_bytes, 0x00020000);
    bool live = r < n_rows;
    int e0 = 0, e1 = 0;
    float si = 0.0f;
    if (live) { e0 = rowptr[r]; e1 = rowptr[r + 1]; si = s1[r]; }
    if (live && long_threshold > 0 && e1 - e0 > long_threshold) { live = false; e1 = e0; }   // the split path owns it

    const float uniform = 1.0f / (float)n_cols;

    // One pass over the row's edges with a running softmax state (max m, sum l, weighted row acc): a piece
    // of LPR edges is scored by its lanes (one edge each), the piece maximum is reduced over the group, the
    // state is rescaled when the maximum moves, then the piece's rows are gathered with weights exp(x - m).
    // Rows of up to LPR edges -- most rows of a citation graph at F = 256 -- never rescale.
    for (int c0 = 0; c0 < n_feat; c0 += TILE) {
        const int col0 = c0 + sub * VEC;
        const unsigned col_off = col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
        float m = -INFINITY, l = 0.0f;              // l: this lane's share of the sum
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
        for (int base = e0; base < e1; base += LPR) {
            const int idx = base + sub;
            int c = 0;
            float x = -INFINITY;
            if (idx < e1) {
                c = col[idx];
                const float xe = leaky(si + s2[c], alpha);
                if (E && c0 == 0) E[idx] = xe;
                if (Elem<T>::to_f32(val[idx]) > 0.0f) x = xe;
            }
            float pmax = x;
#pragma unroll
            for (int off = 1; off < LPR; off <<= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, off));
            if (pmax == -INFINITY) continue;        // no live edge in this piece (uniform across the group)
            const float m_new = fmaxf(m, pmax);
            const float scale = rescale_factor(m, m_new);
            const float p = x == -INFINITY ? 0.0f : expf(x - m_new);
            m = m_new;
            l = l * scale + p;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] *= scale;
            const int n = e1 - base;
#pragma unroll 1
            for (int t0 = 0; t0 < LPR; t0 += UNR) {
                if (t0 >= n) break;
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int t = t0 + u;
                    const int cc = __shfl(c, t, LPR);
                    const float pp = __shfl(p, t, LPR);
                    const unsigned off = (t < n && col_off != kOOB) ? (unsigned)cc * ld_bytes + col_off : kOOB;
                    Gather<T, VEC>::run(acc, pp, rsrc, off);
                }
            }
        }
#pragma unroll
        for (int off = 1; off < LPR; off <<= 1) l += __shfl_xor(l, off);
        const float inv_l = l > 0.0f ? 1.0f / l : 0.0f;
        const bool dead = live && !(l > 0.0f) && fill != nullptr;
        if (S && c0 == 0) {                         // the softmax values, now that the row's (m, l) are known
            for (int idx = e0 + sub; idx < e1; idx += LPR) {
                float p = 0.0f;
                if (dead) p = uniform;
                else if (Elem<T>::to_f32(val[idx]) > 0.0f) p = expf(leaky(si + s2[col[idx]], alpha) - m) * inv_l;
                S[idx] = p;
            }
        }
        if (live && col0 < n_feat) {
            T out[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = dead ? ((col0 + i < n_feat) ? fill[col0 + i] : 0.0f) : acc[i] * inv_l;
#pragma unroll
            for (int i = 0; i < VEC; ++i) out[i] = gat_finish<T>(acc[i], relu, out_scale);
            T *drow = D + r * ldd;
            if (VEC > 1 && vec_store && col0 + VEC <= n_feat) {
                *reinterpret_cast<u32x4 *>(drow + col0) = *reinterpret_cast<const u32x4 *>(out);
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (col0 + i < n_feat) drow[col0 + i] = out[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Long rows (sgx_plan): a hub row of a power-law graph would keep one lane group busy for
// thousands of dependent steps.  Its edges are cut into the plan's 512-edge tasks; one wavefront
// per task keeps a running (max, sum, weighted row sum) per lane group -- rescaled once per piece
// of LPR edges -- and merges its groups; the tasks of a row are then merged in task order
// (m = max m_t, l = sum l_t e^(m_t - m), row = sum acc_t e^(m_t - m) / l): the same softmax, and
// the same bits from run to run.
// ---------------------------------------------------------------------------------------
template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void gat_split_kernel(
    int n_tasks, int n_feat, const int32_t *__restrict__ task_row, const int32_t *__restrict__ task_e0,
    const int32_t *__restrict__ task_e1, const int32_t *__restrict__ col, const T *__restrict__ val,
    const T *__restrict__ Wh, unsigned h_bytes, unsigned ld_bytes, const float *__restrict__ s1,
    const float *__restrict__ s2, float alpha, float *__restrict__ E, float *__restrict__ pacc, int ldp,
    float *__restrict__ pm, float *__restrict__ pl)
{
    constexpr int RPW = 64 / LPR;
    constexpr int TILE = LPR * VEC;
    const int task = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (task >= n_tasks) return;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Wh), 0, h_bytes, 0x00020000);
    const int te0 = task_e0[task], te1 = task_e1[task];
    const float si = s1[task_row[task]];

    for (int c0 = 0; c0 < n_feat; c0 += TILE) {
        const int col0 = c0 + sub * VEC;
        const unsigned col_off = col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
        float m = -INFINITY, l = 0.0f;             // l: this lane's share of the group's sum
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
        for (int base = te0 + grp * LPR; base < te1; base += RPW * LPR) {
            const int idx = base + sub;
            int c = 0;
            float x = -INFINITY;
            if (idx < te1) {
                c = col[idx];
                const float xe = leaky(si + s2[c], alpha);
                if (E && c0 == 0) E[idx] = xe;
                if (Elem<T>::to_f32(val[idx]) > 0.0f) x = xe;
            }
            float pmax = x;
#pragma unroll
            for (int off = 1; off < LPR; off <<= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, off));
            if (pmax == -INFINITY) continue;        // no live edge in this piece (uniform across the group)
            const float m_new = fmaxf(m, pmax);
            const float scale = rescale_factor(m, m_new);
            const float p = x == -INFINITY ? 0.0f : expf(x - m_new);
            m = m_new;
            l = l * scale + p;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] *= scale;
            const int n = te1 - base;
            constexpr int UNR = LPR < 8 ? LPR : 8;
#pragma unroll 1
            for (int t0 = 0; t0 < LPR; t0 += UNR) {
                if (t0 >= n) break;
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int t = t0 + u;
                    const int cc = __shfl(c, t, LPR);
                    const float pp = __shfl(p, t, LPR);
                    Gather<T, VEC>::run(acc, pp, rsrc, (t < n && col_off != kOOB) ? (unsigned)cc * ld_bytes + col_off : kOOB);
                }
            }
        }
#pragma unroll
        for (int off = 1; off < LPR; off <<= 1) l += __shfl_xor(l, off);        // the group's sum
        // merge the lane groups of the wavefront (fixed tree order)
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
            const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
            const float mn = fmaxf(m, m2);
            const float a = rescale_factor(m, mn), b = rescale_factor(m2, mn);
            l = l * a + l2 * b;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = acc[i] * a + __shfl_xor(acc[i], off) * b;
            m = mn;
        }
        if (grp == 0) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (col0 + i < n_feat) pacc[(int64_t)task * ldp + col0 + i] = acc[i];
            if (sub == 0 && c0 == 0) { pm[task] = m; pl[task] = l; }
        }
    }
}

// (pm, pl are [task][head], row_m / row_l [long row][head]; one head: plain [task] / [long row])
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_split_finalize_kernel(
    int n_long, int n_feat, int n_heads, int f_head, const int32_t *__restrict__ long_row,
    const int32_t *__restrict__ long_first, const float *__restrict__ pacc, int ldp, const float *__restrict__ pm,
    const float *__restrict__ pl, T *__restrict__ D, int64_t ldd, int relu, const float *__restrict__ fill,
    float *__restrict__ row_m, float *__restrict__ row_l, float out_scale)
{
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (int64_t)n_long * n_feat) return;
    const int i = (int)(gid / n_feat), j = (int)(gid % n_feat);
    const int h = j / f_head;
    const int t0 = long_first[i], t1 = long_first[i + 1];
    float m = -INFINITY;
    for (int t = t0; t < t1; ++t) m = fmaxf(m, pm[(int64_t)t * n_heads + h]);
    float l = 0.0f, a = 0.0f;
    for (int t = t0; t < t1; ++t) {
        const float w = rescale_factor(pm[(int64_t)t * n_heads + h], m);
        l += pl[(int64_t)t * n_heads + h] * w;
        a += pacc[(int64_t)t * ldp + j] * w;
    }
    float out = l > 0.0f ? a / l : (fill ? fill[j] : 0.0f);
    D[(int64_t)long_row[i] * ldd + j] = gat_finish<T>(out, relu, out_scale);
    if (j % f_head == 0) { row_m[(int64_t)i * n_heads + h] = m; row_l[(int64_t)i * n_heads + h] = l; }
}

// softmax values of the long rows' edges, once the rows' (max, sum) are known: workgroup (i, y) walks
// every gridDim.y-th 256-edge piece of long row i
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_split_softmax_kernel(
    int n_cols, int n_heads, const int32_t *__restrict__ long_row, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, const T *__restrict__ val, const float *__restrict__ s1,
    const float *__restrict__ s2, float alpha, const float *__restrict__ row_m, const float *__restrict__ row_l,
    int filled, float *__restrict__ S)
{
    const int i = blockIdx.x;
    const int row = long_row[i];
    const int e1 = rowptr[row + 1];
    for (int idx = rowptr[row] + blockIdx.y * kBlock + threadIdx.x; idx < e1; idx += gridDim.y * kBlock) {
        const bool pos = Elem<T>::to_f32(val[idx]) > 0.0f;
        const int c = col[idx];
        for (int h = 0; h < n_heads; ++h) {
            const float m = row_m[(int64_t)i * n_heads + h], l = row_l[(int64_t)i * n_heads + h];
            float p = 0.0f;
            if (l > 0.0f) {
                if (pos) p = expf(leaky(s1[(int64_t)row * n_heads + h] + s2[(int64_t)c * n_heads + h], alpha) - m) / l;
            } else if (filled) {
                p = 1.0f / (float)n_cols;
            }
            S[(int64_t)idx * n_heads + h] = p;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Several heads (BASELINE config 5: 8 heads on ogbn-arxiv).  The reference has one head -- its
// `nheads` only widens W (SG.py:1176-1178) -- so this is that single-head formula applied to each
// slice of F_head = n_feat / n_heads columns with its own attention vector
// a_h = attention[h][0 : 2*F_head], outputs concatenated: what n_heads single-head calls on the
// column slices give, in one pass over the edges.  A lane owns VEC columns of one head; it walks
// all edges of its row for that head (scores are 4-byte reads of the per-node, per-head table), so
// no reduction across lanes is needed and each neighbour row is still gathered once.
// ---------------------------------------------------------------------------------------

// TASKS = false: work item = a row (rows over long_threshold edges are left to the tasks).
// TASKS = true:  work item = a task of the plan (an edge chunk of a long row): the lane group leaves the
//                chunk's state -- per head (max, sum) in pm / pl, the unnormalised weighted row in pacc --
//                for gat_split_finalize_kernel; n_rows is then the number of tasks.
template <typename T, int VEC, int LPR, bool TASKS>
__global__ __launch_bounds__(kBlock) void gat_aggregate_heads_kernel(
    int n_rows, int n_cols, int n_feat, int n_heads, int f_head, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, const T *__restrict__ val, const T *__restrict__ Wh, unsigned h_bytes,
    unsigned ld_bytes, const float *__restrict__ s1, const float *__restrict__ s2, float alpha,
    T *__restrict__ D, int64_t ldd, int relu, float *__restrict__ E, float *__restrict__ S, int vec_store,
    const float *__restrict__ fill, int share, int long_threshold, const int32_t *__restrict__ task_row,
    const int32_t *__restrict__ task_e0, const int32_t *__restrict__ task_e1, float *__restrict__ pacc, int ldp,
    float *__restrict__ pm, float *__restrict__ pl, float out_scale)
{
    constexpr int RPW = 64 / LPR;
    constexpr int TILE = LPR * VEC;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const int64_t w = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * RPW + grp;      // work item
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Wh), 0, h_bytes, 0x00020000);
    bool live = w < n_rows;
    int e0 = 0, e1 = 0;
    int64_t r = w;
    if (live) {
        if (TASKS) { r = task_row[w]; e0 = task_e0[w]; e1 = task_e1[w]; }
        else { e0 = rowptr[r]; e1 = rowptr[r + 1]; }
    }
    if (!TASKS && live && long_threshold > 0 && e1 - e0 > long_threshold) { live = false; e1 = e0; }
    const float uniform = 1.0f / (float)n_cols;

    for (int c0 = 0; c0 < n_feat; c0 += TILE) {
        const int col0 = c0 + sub * VEC;
        const bool mine = col0 < n_feat;
        const int h = mine ? col0 / f_head : 0;
        const unsigned col_off = mine ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
        const float si = (live && mine) ? s1[r * n_heads + h] : 0.0f;
        const bool writer = mine && (col0 % f_head == 0);          // one lane per (row, head) writes E / S

        // pass 1: the softmax state of this lane's head over all edges of the row.  The `share` lanes that
        // hold one head (a power of two, adjacent) take every share-th edge each and merge their states.
        float m = -INFINITY, l = 0.0f;
        for (int base = e0; base < e1; base += LPR) {
            const int idx = base + sub;
            int c = 0, pos = 0;
            if (idx < e1) { c = col[idx]; pos = Elem<T>::to_f32(val[idx]) > 0.0f; }
            const int n = e1 - base < LPR ? e1 - base : LPR;
            for (int t0 = 0; t0 < n; t0 += share) {
                const int t = t0 + (sub & (share - 1));
                const int cc = __shfl(c, t, LPR);
                const int pp = __shfl(pos, t, LPR);
                if (t < n && pp && mine) softmax_merge(m, l, leaky(si + s2[(int64_t)cc * n_heads + h], alpha), 1.0f);
            }
        }
        for (int off = 1; off < share; off <<= 1) {
            const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
            softmax_merge(m, l, m2, l2);
        }
        const float inv_l = TASKS ? 1.0f : (l > 0.0f ? 1.0f / l : 0.0f);      // a task stays unnormalised
        const bool dead = !TASKS && live && mine && !(l > 0.0f) && fill != nullptr;

        // pass 2: weighted gather
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
        for (int base = e0; base < e1; base += LPR) {
            const int idx = base + sub;
            int c = 0, pos = 0;
            if (idx < e1) { c = col[idx]; pos = Elem<T>::to_f32(val[idx]) > 0.0f; }
            const int n = e1 - base < LPR ? e1 - base : LPR;
            for (int t = 0; t < n; ++t) {
                const int cc = __shfl(c, t, LPR);
                const int pp = __shfl(pos, t, LPR);
                float x = 0.0f, p = 0.0f;
                if (mine) {
                    x = leaky(si + s2[(int64_t)cc * n_heads + h], alpha);
                    if (pp) p = expf(x - m) * inv_l;
                }
                if (writer) {
                    const int64_t o = (int64_t)(base + t) * n_heads + h;
                    if (E) E[o] = x;
                    if (!TASKS && S) S[o] = dead ? uniform : p;
                }
                Gather<T, VEC>::run(acc, p, rsrc, mine ? (unsigned)cc * ld_bytes + col_off : kOOB);
            }
        }
        if (TASKS) {
            if (live && mine) {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (col0 + i < n_feat) pacc[w * ldp + col0 + i] = acc[i];
                if (writer) { pm[w * n_heads + h] = m; pl[w * n_heads + h] = l; }
            }
            continue;
        }
        if (live && mine) {
            T out[VEC];
            if (dead) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = (col0 + i < n_feat) ? fill[col0 + i] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) out[i] = gat_finish<T>(acc[i], relu, out_scale);
            T *drow = D + r * ldd;
            if (VEC > 1 && vec_store && col0 + VEC <= n_feat) {
                *reinterpret_cast<u32x4 *>(drow + col0) = *reinterpret_cast<const u32x4 *>(out);
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (col0 + i < n_feat) drow[col0 + i] = out[i];
            }
        }
    }
}

// (the scores are in the scratch already; rows over the cut of the plan go through its tasks and are merged in task order)
template <typename T, int VEC, int LPR>
int one_pass(const sgx_gat_args &a)
{
    const int rows_per_block = (64 / LPR) * (kBlock / 64);
    const unsigned grid = (unsigned)((a.n_rows + rows_per_block - 1) / rows_per_block);
    const sgx_gat_scratch &L = a.lay;
    const float *s1 = a.scratch + L.s1, *s2 = a.scratch + L.s2;
    const sgx_plan *p = a.plan;
    const int thr = (p && p->n_long > 0) ? p->long_threshold : 0;
    float *pacc = a.scratch + L.pacc, *pm = a.scratch + L.pm, *pl = a.scratch + L.pl;          // (read and written only when thr > 0)
    float *row_m = a.scratch + L.row_m, *row_l = a.scratch + L.row_l;
    if (a.n_heads > 1) {
        const int f_head = a.n_feat / a.n_heads;
        // lanes per head; they share the softmax pass when that is a power of two that divides the lane
        // group and no head straddles a column tile (otherwise every lane walks all edges itself)
        const int lanes_per_head = f_head / VEC;
        const bool pow2 = lanes_per_head > 0 && (lanes_per_head & (lanes_per_head - 1)) == 0;
        const int share = (f_head % VEC == 0 && pow2 && lanes_per_head <= LPR) ? lanes_per_head : 1;
        hipLaunchKernelGGL((gat_aggregate_heads_kernel<T, VEC, LPR, false>), dim3(grid), dim3(kBlock), 0, a.stream, a.n_rows,
                           a.uniform_n, a.n_feat, a.n_heads, f_head, a.rowptr, a.col, (const T *)a.val, (const T *)a.Wh,
                           a.h_bytes, a.ld_bytes, s1, s2, a.alpha, (T *)a.D, a.ldd, a.relu, a.E, a.S, a.vec_store, a.fill,
                           share, thr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, a.out_scale);
        SGX_LAUNCH_CHECK();
        if (thr > 0) {
            const unsigned tgrid = (unsigned)((p->n_tasks + rows_per_block - 1) / rows_per_block);
            hipLaunchKernelGGL((gat_aggregate_heads_kernel<T, VEC, LPR, true>), dim3(tgrid), dim3(kBlock), 0, a.stream,
                               p->n_tasks, a.uniform_n, a.n_feat, a.n_heads, f_head, a.rowptr, a.col, (const T *)a.val,
                               (const T *)a.Wh, a.h_bytes, a.ld_bytes, s1, s2, a.alpha, (T *)a.D, a.ldd, a.relu, a.E, nullptr,
                               a.vec_store, nullptr, share, 0, p->task_row, p->task_e0, p->task_e1, pacc, L.ldp, pm, pl,
                               a.out_scale);
            SGX_LAUNCH_CHECK();
        }
    } else if (thr > 0) {
        hipLaunchKernelGGL((gat_split_kernel<T, VEC, LPR>), dim3((p->n_tasks + kBlock / 64 - 1) / (kBlock / 64)),
                           dim3(kBlock), 0, a.stream, p->n_tasks, a.n_feat, p->task_row, p->task_e0, p->task_e1, a.col,
                           (const T *)a.val, (const T *)a.Wh, a.h_bytes, a.ld_bytes, s1, s2, a.alpha, a.E, pacc, L.ldp, pm, pl);
        SGX_LAUNCH_CHECK();
    }
    if (thr > 0) {          // the tasks of a long row merged in task order, then its softmax values
        const int64_t total = (int64_t)p->n_long * a.n_feat;
        hipLaunchKernelGGL((gat_split_finalize_kernel<T>), dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           a.stream, p->n_long, a.n_feat, a.n_heads, a.n_feat / a.n_heads, p->long_row, p->long_first, pacc, L.ldp,
                           pm, pl, (T *)a.D, a.ldd, a.relu, a.fill, row_m, row_l, a.out_scale);
        SGX_LAUNCH_CHECK();
        if (a.S) {
            hipLaunchKernelGGL((gat_split_softmax_kernel<T>), dim3(p->n_long, 16), dim3(kBlock), 0, a.stream, a.uniform_n,
                               a.n_heads, p->long_row, a.rowptr, a.col, (const T *)a.val, s1, s2, a.alpha, row_m, row_l,
                               a.fill != nullptr, a.S);
            SGX_LAUNCH_CHECK();
        }
    }
    if (a.n_heads == 1) {
        hipLaunchKernelGGL((gat_aggregate_kernel<T, VEC, LPR>), dim3(grid), dim3(kBlock), 0, a.stream, a.n_rows, a.uniform_n,
                           a.n_feat, a.rowptr, a.col, (const T *)a.val, (const T *)a.Wh, a.h_bytes, a.ld_bytes, s1, s2, a.alpha,
                           (T *)a.D, a.ldd, a.relu, a.E, a.S, a.vec_store, a.fill, thr, a.out_scale);
        SGX_LAUNCH_CHECK();
    }
    return SGX_OK;
}

}  // namespace

int sgx_gat_one_pass(const sgx_gat_args &a)
{
    return sgx_gat_dispatch(a, [&](auto t, auto vec, auto lpr) {
        return one_pass<decltype(t), decltype(vec)::value, decltype(lpr)::value>(a);
    });
}
