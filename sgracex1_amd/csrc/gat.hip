// GAT aggregation for gfx950 (the GAT bitstream has no public HLS source; the arithmetic is the reference's CPU
// emulation, SG.py:309-314 and :634-661):
//     s1_i = Wh_i . a[:F]      s2_j = Wh_j . a[F:]
//     e_ij = LeakyReLU_alpha(s1_i + s2_j)            for stored edges with values[e] > 0
//     alpha_ij = softmax_j(e_ij)                     (rows of the masked dense matrix)
//     D_i = act( sum_j alpha_ij Wh_j )
// The emulation builds dense N x N matrices; here the softmax runs over the CSR row.
// Rows with no positive edge: the emulation's masked dense row is constant (-9e15 everywhere,
// SG.py:638-641), its softmax uniform over all N nodes, so the row receives the mean of all rows
// of Wh.  sym_norm2's self loops (SG.py:42) keep the plain path away from this case, the quantised
// adjacency does not (small values round to 0).  `fill_dead_rows` selects that result (one more
// pass over Wh for the column means); without it such rows produce 0.
//
// This file: the C ABI entries and their argument checks, the layout of the scratch buffer, the score pre-pass, the
// dead-row mean / sgx_col_sums, and the choice of the form that aggregates:
//     gat_one_pass.hip   one walk per row with a running softmax state (no plan needed)
//     gat_alpha.hip      two stages, stage A by rows: the softmax weights of the stored entries
//     gat_scan.hip       stage A in entry order (rows up to the plan's cut)
//     gat_weighted.hip   stage B: the aggregation with those weights
//     gat_fused.hip      one walk that forms the neighbours' scores from the rows it gathers (no E / S outputs)
#include "gat_device.h"

#include <stdlib.h>

namespace {

template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void gat_scores_kernel(int n_rows, int n_feat, const T *__restrict__ Wh, int64_t ldh,
                                                           const T *__restrict__ att, float *__restrict__ s1,
                                                           float *__restrict__ s2, int vec_ok)
{
    constexpr int RPW = 64 / LPR;
    constexpr int TILE = LPR * VEC;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const int64_t r = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * RPW + grp;
    float p1 = 0.0f, p2 = 0.0f;
    if (r < n_rows) {
        for (int c0 = sub * VEC; c0 < n_feat; c0 += TILE) {
            T h[VEC];
            if (VEC > 1 && vec_ok && c0 + VEC <= n_feat) {
                *reinterpret_cast<u32x4 *>(h) = *reinterpret_cast<const u32x4 *>(Wh + r * ldh + c0);
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) h[i] = (c0 + i < n_feat) ? Wh[r * ldh + c0 + i] : (T)0;
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                if (c0 + i < n_feat) {
                    p1 = __builtin_fmaf(Elem<T>::to_f32(h[i]), Elem<T>::to_f32(att[c0 + i]), p1);
                    p2 = __builtin_fmaf(Elem<T>::to_f32(h[i]), Elem<T>::to_f32(att[n_feat + c0 + i]), p2);
                }
            }
        }
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) {
        p1 += __shfl_xor(p1, off);
        p2 += __shfl_xor(p2, off);
    }
    if (r < n_rows && sub == 0) { s1[r] = p1; s2[r] = p2; }
}

// Several heads (BASELINE config 5: 8 heads on ogbn-arxiv).  The reference has one head -- its
// `nheads` only widens W (SG.py:1176-1178) -- so this is that single-head formula applied to each
// slice of F_head = n_feat / n_heads columns with its own attention vector
// a_h = attention[h][0 : 2*F_head], outputs concatenated: what n_heads single-head calls on the
// column slices give.  The scores are a table per (node, head).
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_scores_heads_kernel(int n_cols, int n_heads, int f_head,
                                                                 const T *__restrict__ Wh, int64_t ldh,
                                                                 const T *__restrict__ att, float *__restrict__ s1,
                                                                 float *__restrict__ s2)
{
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (int64_t)n_cols * n_heads) return;
    const int64_t r = gid / n_heads;
    const int h = (int)(gid - r * n_heads);
    const T *w = Wh + r * ldh + (int64_t)h * f_head;
    const T *a = att + (int64_t)h * 2 * f_head;
    float p1 = 0.0f, p2 = 0.0f;
    for (int i = 0; i < f_head; ++i) {
        const float v = Elem<T>::to_f32(w[i]);
        p1 = __builtin_fmaf(v, Elem<T>::to_f32(a[i]), p1);
        p2 = __builtin_fmaf(v, Elem<T>::to_f32(a[f_head + i]), p2);
    }
    s1[gid] = p1;
    s2[gid] = p2;
}

// Scores Wh.a1, Wh.a2 per (node, head) with the rows read 16 bytes per lane: a lane keeps the attention fragments of
// its columns in registers and walks rows grid-stride; the lanes of a head (F_head / VEC of them, a power of two) fold
// their partial dot products with shuffles.  One tile of LPR x VEC columns covers the row.
template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void gat_scores_rows_kernel(int n_rows, int n_feat, int n_heads, int f_head,
                                                                const T *__restrict__ Wh, int64_t ldh,
                                                                const T *__restrict__ att, float *__restrict__ s1,
                                                                float *__restrict__ s2)
{
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, sub = lane % LPR, grp = lane / LPR;
    const int col0 = sub * VEC;
    const bool mine = col0 < n_feat;
    const int h = mine ? col0 / f_head : 0, j0 = mine ? col0 - h * f_head : 0;
    const int lanes_per_head = f_head / VEC;
    // the lane's fragments of the attention vectors: one 16-byte load each where they are aligned (element loads were
    // 2 VEC memory instructions per wavefront ahead of its 4 row loads -- with one wavefront per 8 rows, most of the kernel)
    float a1[VEC], a2[VEC];
    const T *p1 = att + (int64_t)h * 2 * f_head + j0, *p2 = p1 + f_head;
    if (((reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2)) % 16) == 0 && VEC * sizeof(T) == 16) {
        union { u32x4 v; T e[VEC]; } u1, u2;
        u1.v = mine ? *reinterpret_cast<const u32x4 *>(p1) : u32x4{0u, 0u, 0u, 0u};
        u2.v = mine ? *reinterpret_cast<const u32x4 *>(p2) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            a1[i] = mine ? Elem<T>::to_f32(u1.e[i]) : 0.0f;
            a2[i] = mine ? Elem<T>::to_f32(u2.e[i]) : 0.0f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            a1[i] = mine ? Elem<T>::to_f32(p1[i]) : 0.0f;
            a2[i] = mine ? Elem<T>::to_f32(p2[i]) : 0.0f;
        }
    }
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (kBlock / 64);
    // kU row groups per pass, their loads requested before the first is reduced (one at a time was a round trip to
    // memory per 512 bytes: 35 us for the 87 MB of the ogbn-arxiv shape)
    constexpr int kU = 4;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Wh), 0, (unsigned)(((int64_t)(n_rows - 1) * ldh + n_feat) * (int64_t)sizeof(T)), 0x00020000);
    for (int64_t r0 = wave * (RPW * kU); r0 < n_rows; r0 += n_waves * (RPW * kU)) {
        u32x4 raw[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t r = r0 + u * RPW + grp;
            raw[u] = __builtin_amdgcn_raw_buffer_load_b128(
                rsrc, (r < n_rows && mine) ? (unsigned)((r * ldh + col0) * (int64_t)sizeof(T)) : kOOB, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t r = r0 + u * RPW + grp;
            union { u32x4 v; T e[VEC]; } x;
            x.v = raw[u];
            float p1 = 0.0f, p2 = 0.0f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float xv = Elem<T>::to_f32(x.e[i]);
                p1 = __builtin_fmaf(xv, a1[i], p1);
                p2 = __builtin_fmaf(xv, a2[i], p2);
            }
            for (int off = 1; off < lanes_per_head; off <<= 1) {
                p1 += __shfl_xor(p1, off);
                p2 += __shfl_xor(p2, off);
            }
            if (r < n_rows && mine && (sub % lanes_per_head) == 0) {
                s1[r * n_heads + h] = p1;
                s2[r * n_heads + h] = p2;
            }
        }
    }
}

// Column means of Wh in two fixed-order stages: slab sums, then the slabs added in order.
constexpr int kMeanSlabs = 512;

template <typename T>
__global__ __launch_bounds__(kBlock) void col_sum_slab_kernel(int n_rows, int n_feat, const T *__restrict__ Wh, int64_t ldh,
                                                             float *__restrict__ partial)
{
    const int rows_per = (n_rows + kMeanSlabs - 1) / kMeanSlabs;
    const int r0 = blockIdx.x * rows_per;
    const int r1 = r0 + rows_per < n_rows ? r0 + rows_per : n_rows;
    for (int j = threadIdx.x; j < n_feat; j += kBlock) {
        float s = 0.0f;
        for (int r = r0; r < r1; ++r) s += Elem<T>::to_f32(Wh[(int64_t)r * ldh + j]);
        partial[(int64_t)blockIdx.x * n_feat + j] = s;
    }
}

// the slabs added in slab order; n_rows != 0: the column means (a true division), 0: the sums
__global__ __launch_bounds__(kBlock) void col_sum_finish_kernel(int n_feat, const float *__restrict__ partial, float *__restrict__ out,
                                                               int n_rows)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_feat) return;
    float s = 0.0f;
    // (eight slabs requested at a time, added in slab order: one load in flight per thread made this 512 round trips)
    static_assert(kMeanSlabs % 8 == 0, "");
    for (int b0 = 0; b0 < kMeanSlabs; b0 += 8) {
        float v[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) v[b] = partial[(int64_t)(b0 + b) * n_feat + j];
#pragma unroll
        for (int b = 0; b < 8; ++b) s += v[b];
    }
    out[j] = n_rows ? s / (float)n_rows : s;
}

// out = the column sums of X's rows, divided by `divisor` rows unless that is 0; slabs: kMeanSlabs x n_feat floats
int col_sums_launch(int dtype, int n_rows, int n_feat, const void *X, int64_t ldx, float *slabs, float *out, int divisor, hipStream_t s)
{
    if (dtype == SGX_F16)
        hipLaunchKernelGGL(col_sum_slab_kernel<f16>, dim3(kMeanSlabs), dim3(kBlock), 0, s, n_rows, n_feat, (const f16 *)X, ldx, slabs);
    else
        hipLaunchKernelGGL(col_sum_slab_kernel<float>, dim3(kMeanSlabs), dim3(kBlock), 0, s, n_rows, n_feat, (const float *)X, ldx, slabs);
    SGX_LAUNCH_CHECK();
    hipLaunchKernelGGL(col_sum_finish_kernel, dim3((n_feat + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n_feat, slabs, out, divisor);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

// heads of a whole number of 64-column groups: the X.W kernel of a layer may leave the scores as one partial per
// (row, group) for gat_scores_combine_kernel to add up
bool score_partials_possible(int n_feat, int n_heads) { return n_heads >= 1 && n_feat % n_heads == 0 && (n_feat / n_heads) % 64 == 0; }
bool uses_split(const sgx_plan *plan) { return plan && plan->n_long > 0; }
// the two-stage form needs the stored-entry count on the host (a plan carries it) and 32-bit offsets into the weights
bool two_stage_ok(const sgx_plan *plan, int n_heads)
{
    if (sgx_tune().gat_one_pass) return false;           // tuning override: the one-pass kernels
    return plan && plan->nnz > 0 && (unsigned long long)plan->nnz * (unsigned long long)n_heads < (1ull << 30) &&
           (unsigned long long)plan->n_rows * (unsigned long long)n_heads < (1ull << 30);
}

// Stage A's short rows in entry order (gat_scan.hip) instead of 8 rows per wavefront?
// Measured (tools/gat_probe.py, round 3): on a power-law graph one head's short rows take 146 us in entry order against
// 240 us as 8-row wavefronts (29 M-entry R-MAT, 11 M entries in rows up to 256); with 8 heads the log-step scans cost
// six times the vector instructions of the per-row lanes' running maximum and sum (ogbn-arxiv shape 113 against 69 us),
// and on a uniform graph the 8-row wavefronts have no idle lanes to win back.  The rule looks at the plan alone, not at
// the number of heads: entry order on a plan whose short rows are scheduled in degree order -- the plan's own sign of
// rows of very unequal length.
bool gat_scan_wanted(const sgx_plan *p)
{
    const int mode = sgx_tune().gat_scan;          // tuning override: 0 = never, 1 = by shape, 2 = wherever the plan allows
    if (mode == 0 || !sgx_gat_scan_applicable(p)) return false;
    return mode == 2 || p->row_order != nullptr;
}

// The score pre-pass: s1 / s2 of every row of the table into the scratch
template <typename T, int VEC, int LPR>
int gat_scores(const sgx_gat_args &a)
{
    const int rows_per_block = (64 / LPR) * (kBlock / 64);
    const unsigned grid_s = (unsigned)((a.n_cols + rows_per_block - 1) / rows_per_block);
    const int f_head = a.n_feat / a.n_heads;
    float *s1 = a.scratch + a.lay.s1, *s2 = a.scratch + a.lay.s2;
    const int lanes_per_head = VEC > 1 ? f_head / VEC : 0;
    if (a.scores_ready) {
        // (nothing to launch)
    } else if (a.lay.has_two_stage && VEC > 1 && a.vec_ok && a.n_feat <= LPR * VEC && f_head % VEC == 0 && lanes_per_head >= 1 &&
               lanes_per_head <= LPR && (lanes_per_head & (lanes_per_head - 1)) == 0 &&
               (unsigned long long)a.n_cols * (unsigned long long)a.ldh * sizeof(T) <= kOOBRow) {    // (32-bit buffer offsets, as sgx_spmm_table_big)
        int64_t blocks = ((int64_t)a.n_cols + rows_per_block - 1) / rows_per_block;
        if (blocks > 256 * 8) blocks = 256 * 8;
        hipLaunchKernelGGL((gat_scores_rows_kernel<T, VEC, LPR>), dim3((unsigned)blocks), dim3(kBlock), 0, a.stream, a.n_cols,
                           a.n_feat, a.n_heads, f_head, (const T *)a.Wh, a.ldh, (const T *)a.att, s1, s2);
    } else if (a.n_heads > 1) {
        const int64_t pairs = (int64_t)a.n_cols * a.n_heads;
        hipLaunchKernelGGL((gat_scores_heads_kernel<T>), dim3((unsigned)((pairs + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           a.stream, a.n_cols, a.n_heads, f_head, (const T *)a.Wh, a.ldh, (const T *)a.att, s1, s2);
    } else {
        hipLaunchKernelGGL((gat_scores_kernel<T, VEC, LPR>), dim3(grid_s), dim3(kBlock), 0, a.stream, a.n_cols, a.n_feat,
                           (const T *)a.Wh, a.ldh, (const T *)a.att, s1, s2, a.vec_ok);
    }
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

// =======================================================================================
// Two-stage form (used whenever a plan tells the stored-entry count): the softmax weights first, then a plain
// weighted aggregation.
// Why: the one-pass kernels (gat_one_pass.hip) chain three dependent memory latencies per piece (column -> score -> rows) and carry a
// softmax state through every step; on the ogbn-arxiv shape they take 0.27 ms (8 heads 0.41) against 0.18 ms for the
// plain aggregate of the same rows, and hub rows multiply that (R-MAT arxiv shape: 8 heads 1.08 ms).  Stage A moves
// ~14 bytes per edge, stage B is the plain aggregate.
// =======================================================================================
int gat_two_stage(const sgx_gat_args &a)
{
    const sgx_plan *p = a.plan_any;
    const sgx_gat_scratch &L = a.lay;
    // One walk pays while a head spans few lanes -- every lane of a head forms the piece's 8 scores and exponentials itself, and
    // a head wider than a DPP row half sums its dots through LDS permutes (measured, tools/gat_probe.py: 8 heads x 32 columns
    // 0.286 -> 0.234 ms on the arxiv shape, one head of 64 columns 0.80 -> 0.70 ms and 8 heads 1.94 -> 0.74 ms on a 29 M-entry
    // R-MAT graph, 2 heads x 128 columns = 16 lanes 0.252 -> 0.230 ms; one head of 256 columns = 32 lanes 0.235 -> 0.254 ms: the
    // two stages stay).  SGX_GAT_FUSED = 0 / 2: never / wherever it applies.
    const int vec = a.vec_ok ? (int)(16 / sgx_elem_size(a.dtype)) : 1;
    const int lanes_of_a_head = (a.n_feat / a.n_heads) / vec;
    const bool fused_pays = sgx_tune().gat_fused == 2 || (sgx_tune().gat_fused == 1 && lanes_of_a_head <= 16);
    if (!a.E && !a.S && fused_pays && a.vec_ok && sgx_gat_fused_applicable(a.dtype, a.n_feat, a.n_heads, a.lpr)) {
        // no side outputs wanted: one walk over the rows, the neighbours' scores formed from the rows it gathers (gat_fused.hip)
        sgx_gat_fused_args f{};
        f.dtype = a.dtype; f.lpr = a.lpr; f.relu = a.relu; f.n_feat = a.n_feat; f.n_heads = a.n_heads;
        f.n_rows = a.n_rows; f.plan = p; f.vec_store = a.vec_store; f.ldp = L.ldp;
        f.alpha = a.alpha; f.out_scale = a.out_scale;
        f.rowptr = a.rowptr; f.col = a.col;
        f.val = a.val; f.Wh = a.Wh; f.att = a.att; f.h_bytes = a.h_bytes; f.ld_bytes = a.ld_bytes;
        f.s1 = a.scratch + L.s1; f.fill = a.fill; f.D = a.D; f.ldd = a.ldd;
        f.pacc = a.scratch + L.pacc; f.pm = a.scratch + L.pm; f.pl = a.scratch + L.pl; f.stream = a.stream;
        return sgx_gat_fused(f);
    }
    float *W = a.S ? a.S : a.scratch + L.weights;          // the weights are the S output where the caller wants it
    const int rc = sgx_gat_alpha_stage(a, W, gat_scan_wanted(p));
    if (rc != SGX_OK) return rc;
    return sgx_gat_weighted(a, W);
}

// s[r][h] = the groups of head h added in the order of the scores kernel's lane tree: (g0 + g1) + (g2 + g3) ...
__global__ __launch_bounds__(kBlock) void gat_scores_combine_kernel(int64_t n_pairs, int n_heads, int groups_per_head, int n_groups,
                                                                    const float *__restrict__ sp1, const float *__restrict__ sp2,
                                                                    float *__restrict__ s1, float *__restrict__ s2)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pairs) return;
    const int64_t r = i / n_heads;
    const int h = (int)(i % n_heads);
    const float *p1 = sp1 + r * n_groups + (int64_t)h * groups_per_head, *p2 = sp2 + r * n_groups + (int64_t)h * groups_per_head;
    float a1[8], a2[8];                              // (up to 512 columns per head)
    for (int g = 0; g < groups_per_head; ++g) { a1[g] = p1[g]; a2[g] = p2[g]; }
    for (int width = 1; width < groups_per_head; width <<= 1)
        for (int g = 0; g + width < groups_per_head; g += 2 * width) { a1[g] += a1[g + width]; a2[g] += a2[g + width]; }
    s1[i] = a1[0];
    s2[i] = a2[0];
}

}  // namespace

// Where everything lies in the aggregate's scratch, and how much of it there is: the one statement of both.
sgx_gat_scratch sgx_gat_scratch_layout(int n_cols, int n_feat, int n_heads, int fill_dead_rows, const sgx_plan *plan)
{
    if (n_heads < 1) n_heads = 1;
    sgx_gat_scratch L{};
    size_t at = 0;
    auto take = [&at](size_t floats) { const size_t off = at; at += floats; return off; };
    L.s1 = take((size_t)n_cols * n_heads);
    L.s2 = take((size_t)n_cols * n_heads);
    L.slabs = take(fill_dead_rows ? (size_t)kMeanSlabs * n_feat : 0);
    L.mean = take(fill_dead_rows ? (size_t)n_feat : 0);
    L.has_partials = score_partials_possible(n_feat, n_heads);
    L.sp1 = take(L.has_partials ? (size_t)n_cols * (n_feat / 64) : 0);
    L.sp2 = take(L.has_partials ? (size_t)n_cols * (n_feat / 64) : 0);
    at = sgx_align_up(at, 64);
    L.has_split = uses_split(plan);
    L.ldp = (int)sgx_align_up((size_t)n_feat, 4);
    const size_t n_tasks = L.has_split ? plan->n_tasks : 0, n_long = L.has_split ? plan->n_long : 0;
    L.pacc = take(n_tasks * L.ldp);
    L.pm = take(n_tasks * n_heads);
    L.pl = take(n_tasks * n_heads);
    L.row_m = take(n_long * n_heads);
    L.row_l = take(n_long * n_heads);
    at = sgx_align_up(at, 64);
    L.has_two_stage = two_stage_ok(plan, n_heads);
    L.weights = take(L.has_two_stage ? (size_t)plan->nnz * n_heads : 0);
    L.dead = take(L.has_two_stage ? ((size_t)plan->n_rows + 3) / 4 + 16 : 0);
    L.total = at;
    return L;
}

// Whether a layer may have its X.W kernel form the attention scores in its epilogue (xw_dense.hip) and hand them to
// sgx_gat_aggregate_ep as scores_ready: the two-stage form must be the one that runs, and a head must be the 32 columns a
// lane quad of the MFMA tile holds.
bool sgx_gat_scores_fusable(int dtype, int n_feat, int n_heads, const sgx_plan *plan)
{
    if (n_heads < 1) n_heads = 1;
    if (dtype != SGX_F16 || n_feat % n_heads != 0 || n_feat % 64 != 0 || !two_stage_ok(plan, n_heads) || sgx_tune().gat_no_fused_scores)
        return false;
    const int f_head = n_feat / n_heads;
    return f_head == 32 || f_head % 64 == 0;         // a head = a lane quad's pair of tiles, or whole 64-column groups of a wavefront
}

// the partial scores of sgx_xw_dense_scores (heads of 64 columns and more, lay.sp1 / sp2) added up into lay.s1 / s2
int sgx_gat_scores_combine(float *s_scratch, const sgx_gat_scratch &lay, int n_cols, int n_feat, int n_heads, hipStream_t stream)
{
    if (n_heads < 1) n_heads = 1;
    const int n_groups = n_feat / 64, gph = n_groups / n_heads;
    if (!lay.has_partials || gph < 1 || gph > 8 || (gph & (gph - 1))) return SGX_ERR_UNSUPPORTED;
    const int64_t pairs = (int64_t)n_cols * n_heads;
    hipLaunchKernelGGL(gat_scores_combine_kernel, dim3((unsigned)((pairs + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, pairs, n_heads,
                       gph, n_groups, s_scratch + lay.sp1, s_scratch + lay.sp2, s_scratch + lay.s1, s_scratch + lay.s2);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

extern "C" size_t sgx_gat_scratch_bytes(int n_cols, int n_feat, int n_heads, int fill_dead_rows, const sgx_plan *plan)
{
    if (n_cols < 0 || n_feat < 1) return 0;
    return sgx_align_up(sgx_gat_scratch_layout(n_cols, n_feat, n_heads, fill_dead_rows, plan).total * sizeof(float), 256);
}

extern "C" int sgx_gat_aggregate(int dtype, int relu, int fill_dead_rows, int n_rows, int n_cols, int n_feat, int n_heads,
                                 float alpha,
                                 const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                 const void *Wh, int64_t ldh, const void *attention,
                                 void *D, int64_t ldd, float *E, float *S, const sgx_plan *plan, float *s_scratch,
                                 void *stream)
{
    return sgx_gat_aggregate_ep(dtype, relu, fill_dead_rows, n_rows, n_cols, n_feat, n_heads, alpha, rowPtr, columnIndex, values,
                                Wh, ldh, attention, D, ldd, E, S, plan, s_scratch, (hipStream_t)stream, 0.0f);
}

extern "C" int sgx_gat_aggregate_fill(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha,
                                      const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                      const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd, float *E, float *S,
                                      const float *fill, int64_t n_nodes, const sgx_plan *plan, float *s_scratch, void *stream)
{
    if (fill && (n_nodes < 1 || n_nodes > 0x7FFFFFFF)) return SGX_ERR_SHAPE;
    return sgx_gat_aggregate_ep(dtype, relu, 0, n_rows, n_cols, n_feat, n_heads, alpha, rowPtr, columnIndex, values, Wh, ldh,
                                attention, D, ldd, E, S, plan, s_scratch, (hipStream_t)stream, 0.0f, fill, (int)n_nodes);
}

extern "C" size_t sgx_col_sums_scratch_bytes(int n_feat) { return n_feat < 1 ? 0 : (size_t)kMeanSlabs * n_feat * sizeof(float); }

extern "C" int sgx_col_sums(int dtype, int n_rows, int n_feat, const void *X, int64_t ldx, float *out, float *scratch, void *stream)
{
    if (n_rows < 0 || n_feat < 1 || ldx < n_feat) return SGX_ERR_SHAPE;
    if (!out || !scratch || (n_rows > 0 && !X)) return SGX_ERR_NULL;
    if (dtype != SGX_F16 && dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    return col_sums_launch(dtype, n_rows, n_feat, X, ldx, scratch, out, 0, (hipStream_t)stream);
}

int sgx_gat_aggregate_ep(int dtype, int relu, int fill_dead_rows, int n_rows, int n_cols, int n_feat, int n_heads, float alpha,
                         const int32_t *rowPtr, const int32_t *columnIndex, const void *values, const void *Wh, int64_t ldh,
                         const void *attention, void *D, int64_t ldd, float *E, float *S, const sgx_plan *plan,
                         float *s_scratch, hipStream_t stream, float out_scale, const float *ext_fill, int ext_n, int scores_ready)
{
    if (n_heads < 1) n_heads = 1;
    if (plan && plan->n_rows != n_rows) return SGX_ERR_SHAPE;
    if (n_rows < 0 || n_cols < n_rows || n_feat < 1 || ldh < n_feat || ldd < n_feat) return SGX_ERR_SHAPE;
    if (n_feat % n_heads != 0) return SGX_ERR_SHAPE;
    if (n_rows == 0) return SGX_OK;
    if (!rowPtr || !columnIndex || !values || !Wh || !attention || !D) return SGX_ERR_NULL;
    if (!s_scratch) return SGX_ERR_WORKSPACE;
    if (dtype != SGX_F16 && dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    const size_t es = sgx_elem_size(dtype);
    const unsigned long long table_bytes = (unsigned long long)n_cols * (unsigned long long)ldh * es;
    if (table_bytes >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;
    sgx_gat_args a;
    a.dtype = dtype; a.relu = relu; a.n_rows = n_rows; a.n_cols = n_cols; a.n_feat = n_feat; a.n_heads = n_heads; a.alpha = alpha;
    a.rowptr = rowPtr; a.col = columnIndex; a.val = values; a.Wh = Wh; a.att = attention;
    a.ldh = ldh; a.ldd = ldd; a.h_bytes = (unsigned)table_bytes; a.ld_bytes = (unsigned)(ldh * es);
    a.D = D; a.E = E; a.S = S; a.scratch = s_scratch; a.stream = stream; a.out_scale = out_scale;
    a.lay = sgx_gat_scratch_layout(n_cols, n_feat, n_heads, fill_dead_rows, plan);
    a.scores_ready = scores_ready && a.lay.has_two_stage;      // (only the two-stage form takes them; see sgx_gat_scores_fusable)
    if (scores_ready && !a.scores_ready) return SGX_ERR_UNSUPPORTED;
    a.fill = ext_fill;                       // a caller-provided row for dead rows (partitioned graph), or the means below
    a.uniform_n = ext_fill ? ext_n : n_cols;
    a.plan = a.lay.has_split ? plan : nullptr;
    a.plan_any = plan;
    if (fill_dead_rows) {
        float *mean = s_scratch + a.lay.mean;
        const int rc = col_sums_launch(dtype, n_cols, n_feat, Wh, ldh, s_scratch + a.lay.slabs, mean, n_cols, stream);
        if (rc != SGX_OK) return rc;
        a.fill = mean;
    }
    sgx_gat_lane_split(a);
    const int rc = sgx_gat_scores_launch(a);
    if (rc != SGX_OK) return rc;
    return a.lay.has_two_stage ? gat_two_stage(a) : sgx_gat_one_pass(a);
}

// vec_ok, vec_store and lpr (the kernels' template arguments, sgx_gat_dispatch) from the call's pointers and pitches
void sgx_gat_lane_split(sgx_gat_args &a)
{
    const size_t es = sgx_elem_size(a.dtype);
    a.vec_ok = ((uintptr_t)a.Wh % 16 == 0) && ((a.ldh * es) % 16 == 0);
    a.vec_store = ((uintptr_t)a.D % 16 == 0) && ((a.ldd * es) % 16 == 0);
    const int per16 = (int)(16 / es);
    if (a.n_heads > 1 && (a.n_feat / a.n_heads) % per16 != 0) a.vec_ok = 0;      // a lane's 16 bytes must stay inside one head
    a.lpr = sgx_next_pow2(a.vec_ok ? (a.n_feat + per16 - 1) / per16 : a.n_feat);
    if (a.lpr > 64) a.lpr = 64;
}

// the score pre-pass of the call: Wh.a1 / Wh.a2 of every row of the table into a.scratch at a.lay.s1 / s2
int sgx_gat_scores_launch(const sgx_gat_args &a)
{
    return sgx_gat_dispatch(a, [&](auto t, auto vec, auto lpr) {
        return gat_scores<decltype(t), decltype(vec)::value, decltype(lpr)::value>(a);
    });
}

// the dead rows' mean row of Wh (fill_dead_rows) into `mean`: the column-sum pre-pass, slabs added in slab order
size_t sgx_gat_mean_slab_floats(int n_feat) { return (size_t)kMeanSlabs * n_feat; }
int sgx_gat_mean_row(int dtype, int n_cols, int n_feat, const void *Wh, int64_t ldh, float *slabs, float *mean, hipStream_t stream)
{
    return col_sums_launch(dtype, n_cols, n_feat, Wh, ldh, slabs, mean, n_cols, stream);
}
