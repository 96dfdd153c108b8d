// Stage B of the two-stage GAT aggregate (gat.hip): D = act(sum_e alpha_e Wh[col_e]) -- the A.H aggregation with fp32 edge
// weights: the same gather loop as spmm_csr.hip, on the plan's row schedule (row_schedule.h: tasks, lane-group rows, tail).  With several heads a lane reads
// the weight of ITS head for each edge (8 weights per edge lie in one 32-byte piece); each neighbour row is still gathered
// once.  Then the rows stage A flagged as without a live edge receive the fill row.
#include "gat_device.h"

#include <type_traits>

namespace {

// Stage B: D[r][:] = act(sum_e W[e][head of the column] * Wh[col[e]][:]).  Workgroups [0, split_blocks) sum the plan's
// tasks (all lane groups of a wavefront on one task, fp32 partial rows), the others one row per lane group.  HEADS = 0:
// one weight per edge, loaded with the column by the edge's lane and shuffled; HEADS = 1: every lane loads the weight
// of its own head for each edge through a buffer resource (out of range past the row's end: 0, no access).
// SHORT: the degree order's tail of one-step rows (at most 8 edges) 64 rows per wavefront (row_schedule.h, part 3: every
// link of row id -> row pointers -> (column, weight) -> gather is one round trip for 64 rows; the same fma chain per
// output element as the lane-group walk, hence the same bits); workgroups from short_first on.
// The kernel keeps its own text of the schedule's device half (row_schedule.h states the same lines as functions): hipcc's
// code for this kernel moves with any of them -- on a 2.3 M-entry R-MAT graph at 256 columns the aggregate takes 0.199 ms as
// written here, 0.201 / 0.203 / 0.204 with the row walk / the tail tile / the row store through the header, 0.206 with all
// (profiles/row_schedule_gat_weighted_variants.jsonl).  The grid it runs in and the finalize's sum are the header's.
template <typename T, int VEC, int LPR, int HEADS, bool SHORT>
__global__ __launch_bounds__(kBlock) void gat_weighted_kernel(
    int n_work, int n_feat, int n_heads, int f_head, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ W, unsigned w_bytes, const T *__restrict__ Wh, unsigned h_bytes, unsigned ld_bytes,
    T *__restrict__ D, int64_t ldd, int relu, float out_scale, int long_threshold, int vec_store,
    const int32_t *__restrict__ row_order, int split_blocks, int n_tasks, const int32_t *__restrict__ task_e0,
    const int32_t *__restrict__ task_e1, float *__restrict__ partial, int ldp, int n_multi, int short_first,
    const float *__restrict__ task_m, const float *__restrict__ task_l)
{
    constexpr int RPW = 64 / LPR;
    constexpr int TILE = LPR * VEC;
    constexpr int UNR = LPR < 8 ? LPR : 8;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Wh), 0, h_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(W), 0, w_bytes, 0x00020000);

    // the sums of edges [e0, e1) taken `stride` apart in pieces of LPR, for the lane's VEC columns at col0
    // from_scores (a task of a long row whose W still holds stage A's scores, -inf for a masked entry): the weight is
    // exp(score - m) * (1 / l) with the row's merged state, formed here instead of by a pass of its own over W
    auto accumulate = [&](auto from_scores, float *acc, int e0, int e1, int stride, int col0, const float *state_m, const float *state_l) {
        constexpr bool XF = decltype(from_scores)::value;
        const unsigned col_off = col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
        const unsigned my_head = HEADS ? (unsigned)((col0 < n_feat ? col0 : 0) / f_head) : 0u;
        float xm = 0.0f, xinv = 0.0f;
        if constexpr (XF) {
            const float l = state_l[my_head];
            xm = state_m[my_head];
            xinv = l > 0.0f ? 1.0f / l : 0.0f;
        }
        unsigned c_next = 0;
        float a_next = 0.0f;
        auto fetch = [&](int idx, unsigned &c, float &a) {
            c = 0u;
            a = 0.0f;
            if (idx < e1) {
                c = (unsigned)__builtin_nontemporal_load(col + idx);
                if (!HEADS) {
                    a = __builtin_nontemporal_load(W + idx);
                    if constexpr (XF) a = xinv > 0.0f ? exp_weight(a - xm) * xinv : 0.0f;
                }
            }
        };
        fetch(e0 + sub, c_next, a_next);
        for (int base = e0; base < e1; base += stride) {
            const unsigned c = c_next;
            const float a = a_next;
            fetch(base + stride + sub, c_next, a_next);
            const int n = e1 - base;
#pragma unroll 1
            for (int t0 = 0; t0 < LPR; t0 += UNR) {
                if (t0 >= n) break;
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const int t = t0 + u;
                    const unsigned cc = (unsigned)__shfl((int)c, t, LPR);
                    float aa;
                    if (HEADS) {
                        aa = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                 wsrc, t < n ? ((unsigned)(base + t) * (unsigned)n_heads + my_head) * 4u : kOOB, 0, 0));
                        if constexpr (XF) aa = (t < n && xinv > 0.0f) ? exp_weight(aa - xm) * xinv : 0.0f;
                    } else {
                        aa = __shfl(a, t, LPR);
                    }
                    Gather<T, VEC>::run(acc, aa, rsrc, (t < n && col_off != kOOB) ? cc * ld_bytes + col_off : kOOB);
                }
            }
        }
    };

    if ((int)blockIdx.x < split_blocks) {
        const int task = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
        if (task >= n_tasks) return;
        const int e0 = task_e0[task], e1 = task_e1[task];
        for (int c0 = 0; c0 < n_feat; c0 += TILE) {
            const int col0 = c0 + sub * VEC;
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
            if (task_m) accumulate(std::true_type{}, acc, e0 + grp * LPR, e1, 64, col0, task_m + (int64_t)task * n_heads, task_l + (int64_t)task * n_heads);
            else accumulate(std::false_type{}, acc, e0 + grp * LPR, e1, 64, col0, nullptr, nullptr);
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
            if (grp == 0) {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (col0 + i < n_feat) partial[(int64_t)task * ldp + col0 + i] = acc[i];
            }
        }
        return;
    }
    if constexpr (SHORT && LPR >= 8) {
        if ((int)blockIdx.x >= short_first) {
            constexpr int ITER = LPR;
            const int64_t i0 = (int64_t)n_multi + ((int64_t)((int)blockIdx.x - short_first) * (kBlock / 64) + (threadIdx.x >> 6)) * 64;
            if (i0 >= n_work) return;
            const int64_t idx = i0 + lane;
            const bool valid = idx < n_work;
            const int rid = row_order[valid ? idx : (int64_t)n_work - 1];
            const int re0 = rowptr[rid];
            const int rdeg = valid ? rowptr[rid + 1] - re0 : 0;              // at most 8 (the order's last buckets)
            constexpr int CH = 8;                        // iterations per batch of (column, weight) requests
            const int col0 = sub * VEC;
            const unsigned col_off = col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
            const unsigned my_head = HEADS ? (unsigned)((col0 < n_feat ? col0 : 0) / f_head) : 0u;
            for (int it0 = 0; it0 < ITER; it0 += CH) {
            unsigned c[CH];
            float a[CH];
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int s = (it0 + i) * RPW + grp;
                const int se0 = __shfl(re0, s), sdeg = __shfl(rdeg, s);
                const int e = sub < sdeg ? se0 + sub : 0;                    // (unconditional loads: slots past the row read entry 0, masked at use)
                c[i] = (unsigned)__builtin_nontemporal_load(col + e);
                a[i] = HEADS ? 0.0f : __builtin_nontemporal_load(W + e);
            }
#pragma unroll
            for (int it = 0; it < CH; ++it) {
                const int s = (it0 + it) * RPW + grp;
                const int se0 = __shfl(re0, s), sdeg = __shfl(rdeg, s);
                const int64_t rr = __shfl(rid, s);
                const bool live = __shfl((int)valid, s) != 0;
                float acc[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const unsigned cc = (unsigned)__shfl((int)c[it], t, LPR);
                    float aa;
                    if (HEADS)
                        aa = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                 wsrc, t < sdeg ? ((unsigned)(se0 + t) * (unsigned)n_heads + my_head) * 4u : kOOB, 0, 0));
                    else
                        aa = __shfl(a[it], t, LPR);
                    Gather<T, VEC>::run(acc, aa, rsrc, (t < sdeg && col_off != kOOB) ? cc * ld_bytes + col_off : kOOB);
                }
                if (live && col0 < n_feat) {
                    T out[VEC];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) out[i] = gat_finish<T>(acc[i], relu, out_scale);
                    T *drow = D + rr * ldd;
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
            return;
        }
        n_work = n_multi;                    // the walk below takes the rows of two steps and more
    }
    const int row_grid = (SHORT ? short_first : (int)gridDim.x) - split_blocks;
    const int64_t wave = (int64_t)(blockIdx.x - split_blocks) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)row_grid * (kBlock / 64);
    for (int64_t r0 = wave * RPW; r0 < n_work; r0 += n_waves * RPW) {
        int64_t r = r0 + grp;
        int e0 = 0, e1 = 0;
        bool live = r < n_work;
        if (live) {
            if (row_order) r = row_order[r];
            e0 = rowptr[r];
            e1 = rowptr[r + 1];
            if (long_threshold > 0 && e1 - e0 > long_threshold) live = false;
        }
        if (!live) e1 = e0;
        for (int c0 = 0; c0 < n_feat; c0 += TILE) {
            const int col0 = c0 + sub * VEC;
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
            accumulate(std::false_type{}, acc, e0, e1, LPR, col0, nullptr, nullptr);
            if (live && col0 < n_feat) {
                T out[VEC];
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
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gat_weighted_finalize_kernel(
    int n_long, int n_feat, const int32_t *__restrict__ long_row, const int32_t *__restrict__ long_first,
    const float *__restrict__ partial, int ldp, T *__restrict__ D, int64_t ldd, int relu, float out_scale)
{
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (int64_t)n_long * n_feat) return;
    const int l = (int)(gid / n_feat), j = (int)(gid % n_feat);
    const float s = sum_task_partials(partial, ldp, j, long_first[l], long_first[l + 1], 0.0f);   // (the GAT plan cuts at 256 edges)
    D[(int64_t)long_row[l] * ldd + j] = gat_finish<T>(s, relu, out_scale);
}

// rows without a live edge: the row `fill` (the mean of all rows of Wh, SG.py:638-641) and S = 1/N on their edges
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_dead_fill_kernel(
    int n_rows, int n_feat, int n_heads, const unsigned char *__restrict__ dead, const int32_t *__restrict__ rowptr,
    const float *__restrict__ fill, float uniform, T *__restrict__ D, int64_t ldd, int relu, float out_scale,
    float *__restrict__ S)
{
    const int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r >= n_rows || !dead[r]) return;
    const int lane = threadIdx.x & 63;
    for (int j = lane; j < n_feat; j += 64) D[r * ldd + j] = gat_finish<T>(fill[j], relu, out_scale);
    if (S)
        for (int64_t i = (int64_t)rowptr[r] * n_heads + lane; i < (int64_t)rowptr[r + 1] * n_heads; i += 64) S[i] = uniform;
}

template <typename T, int VEC, int LPR>
int weighted(const sgx_gat_args &a, const float *W)
{
    const sgx_plan *p = a.plan_any;
    const sgx_gat_scratch &L = a.lay;
    float *pacc = a.scratch + L.pacc;
    const float *pm = a.scratch + L.pm, *pl = a.scratch + L.pl;
    const unsigned char *dead = reinterpret_cast<const unsigned char *>(a.scratch + L.dead);
    const int ldp = L.ldp;
    const int f_head = a.n_feat / a.n_heads;
    const sgx_row_schedule s = sgx_schedule_rows(p, a.n_rows, LPR, LPR * VEC, a.n_feat, true);
    const unsigned w_bytes = (unsigned)((size_t)p->nnz * a.n_heads * sizeof(float));
#define SGX_GAT_WEIGHTED(HEADS_, SHORT_)                                                                                          \
    hipLaunchKernelGGL((gat_weighted_kernel<T, VEC, LPR, HEADS_, SHORT_>), dim3(s.grid), dim3(kBlock), 0, a.stream, s.n_work, a.n_feat, \
                       a.n_heads, f_head, a.rowptr, a.col, W, w_bytes, (const T *)a.Wh, a.h_bytes, a.ld_bytes, (T *)a.D, a.ldd,      \
                       a.relu, a.out_scale, s.long_threshold, a.vec_store, s.order, s.split_blocks, s.n_tasks, s.task_e0, s.task_e1,  \
                       pacc, ldp, s.n_multi, s.short_first,                                                                       \
                       (s.n_tasks && !a.S) ? pm : nullptr, (s.n_tasks && !a.S) ? pl : nullptr)
    if (a.n_heads > 1) {
        if (s.short_tail) SGX_GAT_WEIGHTED(1, true);
        else SGX_GAT_WEIGHTED(1, false);
    } else {
        if (s.short_tail) SGX_GAT_WEIGHTED(0, true);
        else SGX_GAT_WEIGHTED(0, false);
    }
#undef SGX_GAT_WEIGHTED
    SGX_LAUNCH_CHECK();
    if (s.n_tasks > 0) {
        const int64_t total = (int64_t)p->n_long * a.n_feat;
        hipLaunchKernelGGL((gat_weighted_finalize_kernel<T>), dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           a.stream, p->n_long, a.n_feat, p->long_row, p->long_first, pacc, ldp, (T *)a.D, a.ldd, a.relu,
                           a.out_scale);
        SGX_LAUNCH_CHECK();
    }
    if (a.fill) {
        hipLaunchKernelGGL((gat_dead_fill_kernel<T>), dim3((unsigned)((a.n_rows + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                           a.stream, a.n_rows, a.n_feat, a.n_heads, dead, a.rowptr, a.fill, 1.0f / (float)a.uniform_n, (T *)a.D,
                           a.ldd, a.relu, a.out_scale, a.S);
        SGX_LAUNCH_CHECK();
    }
    return SGX_OK;
}

}  // namespace

int sgx_gat_weighted(const sgx_gat_args &a, const float *W)
{
    return sgx_gat_dispatch(a, [&](auto t, auto vec, auto lpr) {
        return weighted<decltype(t), decltype(vec)::value, decltype(lpr)::value>(a, W);
    });
}
