// Stage A of the two-stage GAT aggregate (gat.hip) by rows: per row the maximum and the sum of its live edges' scores, then
// alpha_e = exp(x_e - m) / l for every stored edge -- the reference's `attention` matrix on the stored entries
// (SG.py:649-653), which is also the S output.  Edge work only: 4-byte score gathers, no rows of Wh.  Per-row kernels for
// one head, 2..64 heads and more than 64 heads; rows over the plan's cut go through its tasks (per-task states merged in
// task order).  gat_scan.hip is the same stage in entry order for the rows up to the cut.
#include "gat_device.h"

namespace {

constexpr int kAlphaLanes = 8;             // lanes per row in stage A (8 rows per wavefront)

// short rows: (max, sum) per head, then the weights; E optional; dead[r] = 1 when the row has no live edge.
// 8 lanes per row split its edges; a row over kCoopEdges8 edges (up to the plan's cut) is taken by the whole wavefront.
constexpr int kCoopEdges8 = 64;

template <typename T, int HB>
__global__ __launch_bounds__(kBlock) void gat_alpha_rows_kernel(
    int n_rows, int n_heads, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    const float *__restrict__ s1, const float *__restrict__ s2, float alpha, int long_threshold,
    float *__restrict__ W, float *__restrict__ E, unsigned char *__restrict__ dead)
{
    constexpr int GL = kAlphaLanes;
    const int lane = threadIdx.x & 63, sub = lane % GL, grp = lane / GL;
    const int64_t r_first = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * (64 / GL);
    const int64_t r = r_first + grp;
    int e0 = 0, e1 = 0;
    bool live_row = r < n_rows;
    if (live_row) { e0 = rowptr[r]; e1 = rowptr[r + 1]; }
    if (live_row && long_threshold > 0 && e1 - e0 > long_threshold) { live_row = false; e1 = e0; }   // the tasks own it
    const int coop_deg = e1 - e0 > kCoopEdges8 ? e1 - e0 : 0;
    const int ce0 = e0;
    if (coop_deg) { live_row = false; e1 = e0; }                                 // taken by the whole wavefront below
    for (int hb0 = 0; hb0 < n_heads; hb0 += HB) {
        float si[HB], m[HB], l[HB];
#pragma unroll
        for (int h = 0; h < HB; ++h) { si[h] = live_row ? s1[r * n_heads + hb0 + h] : 0.0f; m[h] = -INFINITY; l[h] = 0.0f; }
        for (int idx = e0 + sub; idx < e1; idx += GL) {
            const int c = col[idx];
            const bool pos = Elem<T>::to_f32(val[idx]) > 0.0f;
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                const float x = leaky(si[h] + s2[(int64_t)c * n_heads + hb0 + h], alpha);
                if (E) E[(int64_t)idx * n_heads + hb0 + h] = x;
                if (pos) softmax_push(m[h], l[h], x);
            }
        }
#pragma unroll
        for (int off = 1; off < GL; off <<= 1) {
#pragma unroll
            for (int h = 0; h < HB; ++h) softmax_merge(m[h], l[h], __shfl_xor(m[h], off), __shfl_xor(l[h], off));
        }
        for (int idx = e0 + sub; idx < e1; idx += GL) {
            const int c = col[idx];
            const bool pos = Elem<T>::to_f32(val[idx]) > 0.0f;
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                float w = 0.0f;
                if (pos && l[h] > 0.0f) w = expf(leaky(si[h] + s2[(int64_t)c * n_heads + hb0 + h], alpha) - m[h]) / l[h];
                W[(int64_t)idx * n_heads + hb0 + h] = w;
            }
        }
        if (hb0 == 0 && live_row && sub == 0) dead[r] = l[0] > 0.0f ? 0 : 1;      // the mask does not depend on the head
    }
    for (int g = 0; g < 64 / GL; ++g) {
        const int dg = __shfl(coop_deg, g * GL);
        if (dg == 0) continue;                                                     // wave-uniform
        const int ge0 = __shfl(ce0, g * GL), ge1 = ge0 + dg;
        const int64_t gr = r_first + g;
        for (int hb0 = 0; hb0 < n_heads; hb0 += HB) {
            float si[HB], m[HB], l[HB];
#pragma unroll
            for (int h = 0; h < HB; ++h) { si[h] = s1[gr * n_heads + hb0 + h]; m[h] = -INFINITY; l[h] = 0.0f; }
            for (int idx = ge0 + lane; idx < ge1; idx += 64) {
                const int c = col[idx];
                const bool pos = Elem<T>::to_f32(val[idx]) > 0.0f;
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    const float x = leaky(si[h] + s2[(int64_t)c * n_heads + hb0 + h], alpha);
                    if (E) E[(int64_t)idx * n_heads + hb0 + h] = x;
                    if (pos) softmax_push(m[h], l[h], x);
                }
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
                for (int h = 0; h < HB; ++h) softmax_merge(m[h], l[h], __shfl_xor(m[h], off), __shfl_xor(l[h], off));
            }
            for (int idx = ge0 + lane; idx < ge1; idx += 64) {
                const int c = col[idx];
                const bool pos = Elem<T>::to_f32(val[idx]) > 0.0f;
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    float w = 0.0f;
                    if (pos && l[h] > 0.0f) w = expf(leaky(si[h] + s2[(int64_t)c * n_heads + hb0 + h], alpha) - m[h]) / l[h];
                    W[(int64_t)idx * n_heads + hb0 + h] = w;
                }
            }
            if (hb0 == 0 && lane == 0) dead[gr] = l[0] > 0.0f ? 0 : 1;
        }
    }
}

// One head, rows up to 512 edges (every row when the plan cuts at 256): the row's entries live in registers -- 8 per
// lane -- so a row costs two memory round trips (columns and values, then the scores of those columns) whatever its
// length: 8 lanes per row for rows of up to 64 edges (8 rows per wavefront together), the whole wavefront for one row
// of 65..512 edges at a time.  Out-of-range buffer offsets stand in for branches.  Longer rows (a caller's plan with a
// larger cut) take two walks over memory.
template <typename T, int STRIDE>
__device__ __forceinline__ void alpha_row_in_registers(
    bool active, int e0, int deg, int first, int kmax, float si, float alpha, const __amdgpu_buffer_rsrc_t &col_rsrc,
    const __amdgpu_buffer_rsrc_t &val_rsrc, const __amdgpu_buffer_rsrc_t &s2_rsrc, const __amdgpu_buffer_rsrc_t &w_rsrc,
    const __amdgpu_buffer_rsrc_t &e_rsrc, bool want_e, float &l_out)
{
    float x[8];
    unsigned pos = 0u;
    unsigned c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= kmax) break;                                                      // wave-uniform
        const bool ok = active && first + k * STRIDE < deg;
        const unsigned off = ok ? (unsigned)(e0 + first + k * STRIDE) * 4u : kOOB;
        c[k] = __builtin_amdgcn_raw_buffer_load_b32(col_rsrc, off, 0, 0);
        float v;
        if constexpr (sizeof(T) == 2) v = (float)__builtin_bit_cast(T, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(val_rsrc, off >> 1, 0, 0));
        else v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(val_rsrc, off, 0, 0));
        pos |= (ok && v > 0.0f) ? (1u << k) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= kmax) break;
        const bool ok = active && first + k * STRIDE < deg;
        x[k] = leaky(si + __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(s2_rsrc, ok ? c[k] * 4u : kOOB, 0, 0)), alpha);
        if (want_e) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x[k]), e_rsrc,
                                                          ok ? (unsigned)(e0 + first + k * STRIDE) * 4u : kOOB, 0, 0);
    }
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= kmax) break;
        m = (pos >> k) & 1u ? fmaxf(m, x[k]) : m;
    }
#pragma unroll
    for (int off = 1; off < STRIDE; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
    float l = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= kmax) break;
        x[k] = (pos >> k) & 1u ? exp_weight(x[k] - m) : 0.0f;
        l += x[k];
    }
#pragma unroll
    for (int off = 1; off < STRIDE; off <<= 1) l += __shfl_xor(l, off);
    const float inv_l = l > 0.0f ? 1.0f / l : 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= kmax) break;
        const bool ok = active && first + k * STRIDE < deg;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x[k] * inv_l), w_rsrc,
                                              ok ? (unsigned)(e0 + first + k * STRIDE) * 4u : kOOB, 0, 0);
    }
    l_out = l;
}

// (Round 3 tried the several-heads kernel's split here too -- the rows of up to 64 edges in one launch, the longer ones dealt
// out cyclically in a second -- and measured nothing: 1.026 against 1.009 ms on a 29 M-edge R-MAT graph; one launch stays.)
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_alpha_rows_1head_kernel(
    int n_rows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    unsigned nnz_bytes_col, const float *__restrict__ s1, const float *__restrict__ s2, unsigned s_bytes, float alpha,
    int long_threshold, float *__restrict__ W, float *__restrict__ E, unsigned char *__restrict__ dead)
{
    constexpr int GL = 8;
    const int lane = threadIdx.x & 63, sub = lane % GL, grp = lane / GL;
    const int64_t r_first = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * (64 / GL);
    const int64_t r = r_first + grp;
    auto row_of = [&](int g) -> int64_t { return r_first + g; };
    int e0 = 0, e1 = 0;
    if (r < n_rows) { e0 = rowptr[r]; e1 = rowptr[r + 1]; }
    const bool tasked = long_threshold > 0 && e1 - e0 > long_threshold;           // the tasks own it
    const int deg = tasked ? 0 : e1 - e0;
    const __amdgpu_buffer_rsrc_t col_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(col), 0, nnz_bytes_col, 0x00020000);
    const __amdgpu_buffer_rsrc_t val_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(val), 0, (unsigned)(nnz_bytes_col / 4 * sizeof(T)), 0x00020000);
    const __amdgpu_buffer_rsrc_t s2_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(s2), 0, s_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(W, 0, nnz_bytes_col, 0x00020000);
    const __amdgpu_buffer_rsrc_t e_rsrc = __builtin_amdgcn_make_buffer_rsrc(E ? E : W, 0, nnz_bytes_col, 0x00020000);

    // rows of up to 64 edges: 8 lanes each, all 8 rows of the wavefront together
    const bool small = r < n_rows && !tasked && deg <= 64;
    int nm = small ? deg : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) nm = max(nm, __shfl_xor(nm, off));
    nm = __builtin_amdgcn_readfirstlane(nm);
    {
        float l = 0.0f;
        const float si = small ? s1[r] : 0.0f;
        alpha_row_in_registers<T, GL>(small, e0, deg, sub, (nm + GL - 1) / GL, si, alpha, col_rsrc, val_rsrc, s2_rsrc, w_rsrc, e_rsrc,
                                      E != nullptr, l);
        if (small && sub == 0) dead[r] = l > 0.0f ? 0 : 1;
    }
    // rows of 65..512 edges: the whole wavefront, one row at a time
    const int mid_deg = (r < n_rows && !tasked && deg > 64 && deg <= 512) ? deg : 0;
    const int big_deg = (r < n_rows && !tasked && deg > 512) ? deg : 0;
    for (int g = 0; g < 64 / GL; ++g) {
        const int dg = __shfl(mid_deg, g * GL);
        if (dg == 0) continue;                                                     // wave-uniform
        const int ge0 = __shfl(e0, g * GL);
        float l = 0.0f;
        alpha_row_in_registers<T, 64>(true, ge0, dg, lane, (dg + 63) / 64, s1[row_of(g)], alpha, col_rsrc, val_rsrc, s2_rsrc, w_rsrc,
                                      e_rsrc, E != nullptr, l);
        if (lane == 0) dead[row_of(g)] = l > 0.0f ? 0 : 1;
    }
    // rows over 512 edges that the plan did not cut: two walks over memory, whole wavefront
    for (int g = 0; g < 64 / GL; ++g) {
        const int dg = __shfl(big_deg, g * GL);
        if (dg == 0) continue;
        const int ge0 = __shfl(e0, g * GL), ge1 = ge0 + dg;
        const int64_t gr = row_of(g);
        const float si = s1[gr];
        float m = -INFINITY, l = 0.0f;
        for (int idx = ge0 + lane; idx < ge1; idx += 64) {
            const float xk = leaky(si + s2[col[idx]], alpha);
            if (E) E[idx] = xk;
            if (Elem<T>::to_f32(val[idx]) > 0.0f) m = fmaxf(m, xk);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
        for (int idx = ge0 + lane; idx < ge1; idx += 64)
            if (Elem<T>::to_f32(val[idx]) > 0.0f) l += expf(leaky(si + s2[col[idx]], alpha) - m);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) l += __shfl_xor(l, off);
        for (int idx = ge0 + lane; idx < ge1; idx += 64) {
            float w = 0.0f;
            if (Elem<T>::to_f32(val[idx]) > 0.0f && l > 0.0f) w = expf(leaky(si + s2[col[idx]], alpha) - m) / l;
            W[idx] = w;
        }
        if (lane == 0) dead[gr] = l > 0.0f ? 0 : 1;
    }
}

// short rows, several heads: one lane per (row, head), LH = heads rounded up to a power of two lanes per row.  The
// lanes of a row read the same column indices and one contiguous piece of the score / weight rows (LH x 4 bytes).
// A row of up to kAloneEdges edges is taken in ONE pass with everything in registers: its column indices, then its
// scores, are requested together (out-of-range offsets past the row's end: no branches, no access), so a row costs
// two memory round trips whatever its length; maximum, sum and weights follow from the registers.  Longer rows (up to
// the plan's cut) are taken by the whole wavefront one at a time -- a lane per edge, 8 heads in its registers -- with
// the maximum and the sum folded across lanes separately (a max / an add per shuffle instead of a softmax merge).
constexpr int kAloneEdges = 32;

// PART: 0 = everything in one launch; 1 = only the rows of up to kAloneEdges edges (the register pass: a launch of its own
// needs far fewer registers than the two forms together -- more wavefronts in flight for a kernel that is all latency);
// 2 = only the longer rows (the cooperative passes).
template <typename T, int LH, int PART>
__global__ __launch_bounds__(kBlock) void gat_alpha_rows_heads_kernel(
    int n_rows, int n_heads, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const T *__restrict__ val,
    unsigned nnz_bytes_col, const float *__restrict__ s1, const float *__restrict__ s2, unsigned s_bytes, float alpha,
    int long_threshold, float *__restrict__ W, float *__restrict__ E, unsigned char *__restrict__ dead)
{
    constexpr int RPW = 64 / LH;
    constexpr int KB = kAloneEdges;
    const int lane = threadIdx.x & 63, h = lane % LH, grp = lane / LH;
    // PART 2 deals the rows out cyclically (slot g of wavefront w takes row g W + w, W = all wavefronts): the longer rows of
    // a power-law graph sit next to each other, and taken 8 to a wavefront they would queue up behind one another
    const int64_t gwave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (kBlock / 64);
    const int64_t r = PART == 2 ? (int64_t)grp * n_waves + gwave : gwave * RPW + grp;
    const bool head_ok = h < n_heads;
    int e0 = 0, e1 = 0;
    if (r < n_rows) { e0 = rowptr[r]; e1 = rowptr[r + 1]; }
    const bool tasked = long_threshold > 0 && e1 - e0 > long_threshold;           // the tasks own it
    if (tasked) e1 = e0;
    const int deg = e1 - e0;
    const bool alone = r < n_rows && !tasked && deg <= KB;
    const __amdgpu_buffer_rsrc_t col_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(col), 0, nnz_bytes_col, 0x00020000);
    const __amdgpu_buffer_rsrc_t val_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(val), 0, (unsigned)(nnz_bytes_col / 4 * sizeof(T)), 0x00020000);
    const __amdgpu_buffer_rsrc_t s2_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(s2), 0, s_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(W, 0, nnz_bytes_col * (unsigned)n_heads, 0x00020000);
    const __amdgpu_buffer_rsrc_t e_rsrc = __builtin_amdgcn_make_buffer_rsrc(E ? E : W, 0, nnz_bytes_col * (unsigned)n_heads, 0x00020000);

    int nm = alone ? deg : 0;                                                    // the longest such row of the wavefront
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) nm = max(nm, __shfl_xor(nm, off));
    nm = __builtin_amdgcn_readfirstlane(nm);
    if (PART != 2 && nm > 0) {
        const float si = (alone && head_ok) ? s1[r * n_heads + h] : 0.0f;
        float x[KB];
        unsigned pos = 0u;
#pragma unroll
        for (int k0 = 0; k0 < KB; k0 += 8) {
            if (k0 >= nm) break;
            unsigned c[8];
            if constexpr (LH >= 8) {
                // lane j of a row requests entry k0 + j -- one column and one value instruction per 8 entries, 32 contiguous
                // bytes per row, instead of one per entry with the row's lanes all on the same address (every such
                // instruction is 8 rows' lines to look up; the kernel is bound by those look-ups) -- and the row's lanes
                // take the columns from one another; the live flags of the row's 8 entries come out of one ballot
                const bool mine = alone && h < 8 && k0 + h < deg;
                const unsigned off = mine ? (unsigned)(e0 + k0 + h) * 4u : kOOB;
                const unsigned cm = __builtin_amdgcn_raw_buffer_load_b32(col_rsrc, off, 0, 0);
                float v;
                if constexpr (sizeof(T) == 2) {
                    const unsigned short hb = __builtin_amdgcn_raw_buffer_load_b16(val_rsrc, off >> 1, 0, 0);
                    v = (float)__builtin_bit_cast(T, hb);
                } else {
                    v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(val_rsrc, off, 0, 0));
                }
                const unsigned long long live = __ballot(mine && v > 0.0f);
                pos |= ((unsigned)(live >> (grp * LH)) & 0xFFu) << k0;
#pragma unroll
                for (int k = 0; k < 8; ++k) c[k] = (unsigned)__builtin_amdgcn_ds_bpermute((grp * LH + k) * 4, (int)cm);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool ok = alone && head_ok && k0 + k < deg;
                    const unsigned off = ok ? (unsigned)(e0 + k0 + k) * 4u : kOOB;
                    c[k] = __builtin_amdgcn_raw_buffer_load_b32(col_rsrc, off, 0, 0);
                    float v;
                    if constexpr (sizeof(T) == 2) {
                        const unsigned short hb = __builtin_amdgcn_raw_buffer_load_b16(val_rsrc, off >> 1, 0, 0);
                        v = (float)__builtin_bit_cast(T, hb);
                    } else {
                        v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(val_rsrc, off, 0, 0));
                    }
                    pos |= (ok && v > 0.0f) ? (1u << (k0 + k)) : 0u;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool ok = alone && head_ok && k0 + k < deg;
                const float sj = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                     s2_rsrc, ok ? (c[k] * (unsigned)n_heads + (unsigned)h) * 4u : kOOB, 0, 0));
                x[k0 + k] = leaky(si + sj, alpha);
                if (E) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x[k0 + k]), e_rsrc,
                                                             ok ? ((unsigned)(e0 + k0 + k) * (unsigned)n_heads + (unsigned)h) * 4u : kOOB, 0, 0);
            }
        }
        float m = -INFINITY;
#pragma unroll
        for (int k0 = 0; k0 < KB; k0 += 8) {
            if (k0 >= nm) break;
#pragma unroll
            for (int k = 0; k < 8; ++k) m = (pos >> (k0 + k)) & 1u ? fmaxf(m, x[k0 + k]) : m;
        }
        float l = 0.0f;
#pragma unroll
        for (int k0 = 0; k0 < KB; k0 += 8) {
            if (k0 >= nm) break;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float p = (pos >> (k0 + k)) & 1u ? exp_weight(x[k0 + k] - m) : 0.0f;
                x[k0 + k] = p;
                l += p;
            }
        }
        const float inv_l = l > 0.0f ? 1.0f / l : 0.0f;
#pragma unroll
        for (int k0 = 0; k0 < KB; k0 += 8) {
            if (k0 >= nm) break;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool ok = alone && head_ok && k0 + k < deg;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x[k0 + k] * inv_l), w_rsrc,
                                                      ok ? ((unsigned)(e0 + k0 + k) * (unsigned)n_heads + (unsigned)h) * 4u : kOOB, 0, 0);
            }
        }
        if (alone && h == 0) dead[r] = l > 0.0f ? 0 : 1;
    } else if (PART != 2 && alone && h == 0) {
        dead[r] = 1;             // a wavefront whose rows are all empty: they are rows without a live edge all the same
    }
    if (PART == 1) return;

    // the longer rows of this wavefront, one at a time with every lane: a lane per edge, the heads (8 at a time) in its
    // registers; maximum first, then the sum of exp(x - max), then the weights
    const int coop_deg = (!tasked && deg > KB) ? deg : 0;
    const bool vec8 = n_heads % 8 == 0 && (reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(E)) % 16 == 0;
    for (int g = 0; g < RPW; ++g) {
        const int dg = __shfl(coop_deg, g * LH);
        if (dg == 0) continue;                                                     // wave-uniform
        const int ge0 = __shfl(e0, g * LH), ge1 = ge0 + dg;
        const int64_t gr = PART == 2 ? (int64_t)g * n_waves + gwave : gwave * RPW + g;
        if (dg <= 256) {
            // up to 4 edges per lane: the row's scores (8 heads at a time) stay in registers -- columns and values
            // requested together, then the score rows, then maximum, sum and weights without another read
            const int kmax = (dg + 63) / 64;
            unsigned c[4];
            unsigned pv = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= kmax) break;
                const bool ok = lane + 64 * k < dg;
                const unsigned off = ok ? (unsigned)(ge0 + lane + 64 * k) * 4u : kOOB;
                c[k] = __builtin_amdgcn_raw_buffer_load_b32(col_rsrc, off, 0, 0);
                float v;
                if constexpr (sizeof(T) == 2) v = (float)__builtin_bit_cast(T, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(val_rsrc, off >> 1, 0, 0));
                else v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(val_rsrc, off, 0, 0));
                pv |= (ok && v > 0.0f) ? (1u << k) : 0u;
            }
            for (int hb0 = 0; hb0 < n_heads; hb0 += 8) {
                float si[8], m[8], l[8], x[4][8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { si[q] = hb0 + q < n_heads ? s1[gr * n_heads + hb0 + q] : 0.0f; m[q] = -INFINITY; l[q] = 0.0f; }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= kmax) break;
                    const bool ok = lane + 64 * k < dg;
                    load_scores8(s2, ok ? (int64_t)c[k] : 0, n_heads, hb0, vec8, x[k]);
#pragma unroll
                    for (int q = 0; q < 8; ++q) x[k][q] = leaky(si[q] + x[k][q], alpha);
                    if (E && ok) store8(E, ge0 + lane + 64 * k, n_heads, hb0, vec8, x[k]);
                    if ((pv >> k) & 1u) {
#pragma unroll
                        for (int q = 0; q < 8; ++q) m[q] = fmaxf(m[q], x[k][q]);
                    }
                }
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) m[q] = fmaxf(m[q], __shfl_xor(m[q], off));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= kmax) break;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        x[k][q] = (pv >> k) & 1u ? exp_weight(x[k][q] - m[q]) : 0.0f;
                        l[q] += x[k][q];
                    }
                }
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) l[q] += __shfl_xor(l[q], off);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= kmax) break;
#pragma unroll
                    for (int q = 0; q < 8; ++q) x[k][q] = l[q] > 0.0f ? x[k][q] / l[q] : 0.0f;
                    if (lane + 64 * k < dg) store8(W, ge0 + lane + 64 * k, n_heads, hb0, vec8, x[k]);
                }
                if (hb0 == 0 && lane == 0) dead[gr] = l[0] > 0.0f ? 0 : 1;
            }
            continue;
        }
        for (int hb0 = 0; hb0 < n_heads; hb0 += 8) {
            float si[8], m[8], l[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { si[k] = hb0 + k < n_heads ? s1[gr * n_heads + hb0 + k] : 0.0f; m[k] = -INFINITY; l[k] = 0.0f; }
            for (int idx = ge0 + lane; idx < ge1; idx += 64) {
                const int c = col[idx];
                const bool pv = Elem<T>::to_f32(val[idx]) > 0.0f;
                float sc[8];
                load_scores8(s2, c, n_heads, hb0, vec8, sc);
#pragma unroll
                for (int k = 0; k < 8; ++k) sc[k] = leaky(si[k] + sc[k], alpha);
                if (E) store8(E, idx, n_heads, hb0, vec8, sc);
                if (pv) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], sc[k]);
                }
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
                for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], __shfl_xor(m[k], off));
            }
            for (int idx = ge0 + lane; idx < ge1; idx += 64) {
                const int c = col[idx];
                if (Elem<T>::to_f32(val[idx]) > 0.0f) {
                    float sc[8];
                    load_scores8(s2, c, n_heads, hb0, vec8, sc);
#pragma unroll
                    for (int k = 0; k < 8; ++k) l[k] += expf(leaky(si[k] + sc[k], alpha) - m[k]);
                }
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
                for (int k = 0; k < 8; ++k) l[k] += __shfl_xor(l[k], off);
            }
            for (int idx = ge0 + lane; idx < ge1; idx += 64) {
                const int c = col[idx];
                const bool pv = Elem<T>::to_f32(val[idx]) > 0.0f;
                float sc[8];
                load_scores8(s2, c, n_heads, hb0, vec8, sc);
#pragma unroll
                for (int k = 0; k < 8; ++k) sc[k] = (pv && l[k] > 0.0f) ? expf(leaky(si[k] + sc[k], alpha) - m[k]) / l[k] : 0.0f;
                store8(W, idx, n_heads, hb0, vec8, sc);
            }
            if (hb0 == 0 && lane == 0) dead[gr] = l[0] > 0.0f ? 0 : 1;
        }
    }
}

// long rows, step 1: one wavefront per task -- its (max, sum) per head, E of its entries, and the scores themselves left
// in W (-inf for a masked entry), so that step 3 streams them back instead of gathering a second time.  256 entries a
// pass: columns and values requested together, then their score rows (one entry per lane and pass was a chain of two
// memory round trips per 64 entries: 100 us for the 18 M long-row entries of a 29 M-entry R-MAT graph).
template <typename T, int HB>
__global__ __launch_bounds__(kBlock) void gat_alpha_task_stats_kernel(
    int n_tasks, int n_heads, const int32_t *__restrict__ task_row, const int32_t *__restrict__ task_e0,
    const int32_t *__restrict__ task_e1, const int32_t *__restrict__ col, const T *__restrict__ val,
    const float *__restrict__ s1, const float *__restrict__ s2, float alpha, float *__restrict__ E, float *__restrict__ W,
    float *__restrict__ pm, float *__restrict__ pl)
{
    constexpr int U = 4;
    const int task = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (task >= n_tasks) return;
    const int lane = threadIdx.x & 63;
    const int64_t r = task_row[task];
    const int te0 = task_e0[task], te1 = task_e1[task];
    if (te1 <= te0) return;
    const bool vec = HB >= 4 && (reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(E) |
                                 reinterpret_cast<uintptr_t>(W)) % 16 == 0;
    for (int hb0 = 0; hb0 < n_heads; hb0 += HB) {
        float si[HB], m[HB], l[HB];
        load_scores<HB>(s1, r, n_heads, hb0, vec, si);
#pragma unroll
        for (int h = 0; h < HB; ++h) { m[h] = -INFINITY; l[h] = 0.0f; }
        for (int i0 = te0; i0 < te1; i0 += 64 * U) {
            int c[U];
            unsigned live = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + 64 * u + lane, at = min(idx, te1 - 1);
                c[u] = col[at];
                live |= (idx < te1 && Elem<T>::to_f32(val[at]) > 0.0f) ? (1u << u) : 0u;
            }
            float x[U][HB];
#pragma unroll
            for (int u = 0; u < U; ++u) load_scores<HB>(s2, (int64_t)c[u], n_heads, hb0, vec, x[u]);
            float mk[HB];
#pragma unroll
            for (int h = 0; h < HB; ++h) mk[h] = m[h];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + 64 * u + lane;
#pragma unroll
                for (int h = 0; h < HB; ++h) x[u][h] = leaky(si[h] + x[u][h], alpha);
                if (E && idx < te1) store_heads<HB>(E, idx, n_heads, hb0, vec, x[u]);
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    x[u][h] = (live >> u) & 1u ? x[u][h] : -INFINITY;
                    mk[h] = fmaxf(mk[h], x[u][h]);
                }
                if (idx < te1) store_heads<HB>(W, idx, n_heads, hb0, vec, x[u]);
            }
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (mk[h] == -INFINITY) continue;
                float sum = l[h] * rescale_factor(m[h], mk[h]);
#pragma unroll
                for (int u = 0; u < U; ++u) sum += exp_weight(x[u][h] - mk[h]);           // (a masked entry: exp(-inf) = 0)
                l[h] = sum;
                m[h] = mk[h];
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int h = 0; h < HB; ++h) softmax_merge(m[h], l[h], __shfl_xor(m[h], off), __shfl_xor(l[h], off));
        }
        if (lane == 0) {
#pragma unroll
            for (int h = 0; h < HB; ++h) { pm[(int64_t)task * n_heads + hb0 + h] = m[h]; pl[(int64_t)task * n_heads + hb0 + h] = l[h]; }
        }
    }
}

// long rows, step 2: one wavefront per (long row, head) -- its tasks' states merged, 64 at a time in a fixed lane order,
// and the row's state written back over every one of them, so that step 3 can run per TASK and read pm / pl at its own
// index (a thread per row and head walking up to hundreds of tasks one after the other took 38 us)
__global__ __launch_bounds__(kBlock) void gat_alpha_long_merge_kernel(
    int n_long, int n_heads, const int32_t *__restrict__ long_row, const int32_t *__restrict__ long_first,
    float *__restrict__ pm, float *__restrict__ pl, float *__restrict__ row_m, float *__restrict__ row_l,
    unsigned char *__restrict__ dead)
{
    const int64_t pair = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (pair >= (int64_t)n_long * n_heads) return;
    const int lane = threadIdx.x & 63;
    const int i = (int)(pair / n_heads), h = (int)(pair % n_heads);
    const int t0 = long_first[i], t_end = long_first[i + 1];
    float m = -INFINITY, l = 0.0f;
    for (int t = t0 + lane; t < t_end; t += 64) softmax_merge(m, l, pm[(int64_t)t * n_heads + h], pl[(int64_t)t * n_heads + h]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) softmax_merge(m, l, __shfl_xor(m, off), __shfl_xor(l, off));
    m = __shfl(m, 0);                           // (one lane's result for all: the merge is not symmetric in its last bits)
    l = __shfl(l, 0);
    for (int t = t0 + lane; t < t_end; t += 64) { pm[(int64_t)t * n_heads + h] = m; pl[(int64_t)t * n_heads + h] = l; }
    if (lane == 0) {
        row_m[pair] = m;
        row_l[pair] = l;
        if (h == 0) dead[long_row[i]] = l > 0.0f ? 0 : 1;
    }
}

// long rows, step 3: the weights of their entries from the scores step 1 left in W, one wavefront per TASK (the row's
// merged state lies at the task's own index after step 2): a streaming pass, no gathers
__global__ __launch_bounds__(kBlock) void gat_alpha_long_write_kernel(
    int n_tasks, int n_heads, const int32_t *__restrict__ task_e0, const int32_t *__restrict__ task_e1,
    const float *__restrict__ pm, const float *__restrict__ pl, float *__restrict__ W)
{
    constexpr int U = 4;
    const int task = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (task >= n_tasks) return;
    const int lane = threadIdx.x & 63;
    const int64_t f0 = (int64_t)task_e0[task] * n_heads, f1 = (int64_t)task_e1[task] * n_heads;
    if (f1 <= f0) return;
    const float *tm = pm + (int64_t)task * n_heads, *tl = pl + (int64_t)task * n_heads;
    float *Wt = W + f0;
    const int n = (int)(f1 - f0);                                  // (a task's scores: entries x heads, well under 2^31)
    const bool pow2 = (n_heads & (n_heads - 1)) == 0;
    for (int j0 = 0; j0 < n; j0 += 64 * U) {
        float x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = Wt[min(j0 + 64 * u + lane, n - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + 64 * u + lane;
            const int h = pow2 ? (j & (n_heads - 1)) : j % n_heads;        // (the task begins at head 0 of an entry)
            const float m = tm[h], l = tl[h];
            if (j < n) Wt[j] = l > 0.0f ? exp_weight(x[u] - m) * (1.0f / l) : 0.0f;     // (the expression of gat_weighted_kernel's from_scores)
        }
    }
}

template <typename T, int HB>
int alpha_stage(const sgx_gat_args &a, float *W, bool scan)
{
    const sgx_plan *p = a.plan_any;
    const sgx_gat_scratch &L = a.lay;
    const float *s1 = a.scratch + L.s1, *s2 = a.scratch + L.s2;
    float *pm = a.scratch + L.pm, *pl = a.scratch + L.pl, *row_m = a.scratch + L.row_m, *row_l = a.scratch + L.row_l;
    unsigned char *dead = reinterpret_cast<unsigned char *>(a.scratch + L.dead);
    const int thr = p->n_long > 0 ? p->long_threshold : 0;
    const int rows_per_block = (64 / kAlphaLanes) * (kBlock / 64);
    if (scan) {     // the rows up to the cut in entry order (gat_scan.hip); the longer ones below, as ever
        const int rc = sgx_gat_alpha_scan(sizeof(T) == 2 ? SGX_F16 : SGX_F32, a.n_rows, a.n_heads, p, a.rowptr, a.col, a.val, s1, s2,
                                          a.alpha, W, a.E, a.fill ? dead : nullptr, a.stream);
        if (rc != SGX_OK) return rc;
    } else if (a.n_heads == 1) {
        const dim3 grid1((unsigned)((a.n_rows + rows_per_block - 1) / rows_per_block));
        hipLaunchKernelGGL((gat_alpha_rows_1head_kernel<T>), grid1, dim3(kBlock), 0, a.stream, a.n_rows, a.rowptr, a.col,
                           (const T *)a.val, (unsigned)(p->nnz * 4), s1, s2, (unsigned)((size_t)a.n_cols * 4), a.alpha, thr, W, a.E, dead);
    } else if (a.n_heads <= 64) {
        int lh = sgx_next_pow2(a.n_heads);
        const int rpb = (64 / lh) * (kBlock / 64);
        const dim3 grid((unsigned)((a.n_rows + rpb - 1) / rpb));
#define SGX_GAT_LH(L)                                                                                                     \
    case L:                                                                                                               \
        hipLaunchKernelGGL((gat_alpha_rows_heads_kernel<T, L, 1>), grid, dim3(kBlock), 0, a.stream, a.n_rows, a.n_heads,      \
                           a.rowptr, a.col, (const T *)a.val, (unsigned)(p->nnz * 4), s1, s2,                                \
                           (unsigned)((size_t)a.n_cols * a.n_heads * 4), a.alpha, thr, W, a.E, dead);                        \
        if (p->max_degree > kAloneEdges) /* (the second launch serves only rows above that: none on e.g. a uniform graph) */ \
            hipLaunchKernelGGL((gat_alpha_rows_heads_kernel<T, L, 2>), grid, dim3(kBlock), 0, a.stream, a.n_rows, a.n_heads,  \
                               a.rowptr, a.col, (const T *)a.val, (unsigned)(p->nnz * 4), s1, s2,                            \
                               (unsigned)((size_t)a.n_cols * a.n_heads * 4), a.alpha, thr, W, a.E, dead);                    \
        break;
        switch (lh) {
            SGX_GAT_LH(2) SGX_GAT_LH(4) SGX_GAT_LH(8) SGX_GAT_LH(16) SGX_GAT_LH(32) SGX_GAT_LH(64)
        }
#undef SGX_GAT_LH
    } else {
        hipLaunchKernelGGL((gat_alpha_rows_kernel<T, HB>), dim3((unsigned)((a.n_rows + rows_per_block - 1) / rows_per_block)),
                           dim3(kBlock), 0, a.stream, a.n_rows, a.n_heads, a.rowptr, a.col, (const T *)a.val, s1, s2, a.alpha, thr,
                           W, a.E, dead);
    }
    SGX_LAUNCH_CHECK();
    if (thr > 0) {
        hipLaunchKernelGGL((gat_alpha_task_stats_kernel<T, HB>), dim3((p->n_tasks + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock),
                           0, a.stream, p->n_tasks, a.n_heads, p->task_row, p->task_e0, p->task_e1, a.col, (const T *)a.val, s1,
                           s2, a.alpha, a.E, W, pm, pl);
        SGX_LAUNCH_CHECK();
        const int64_t pairs = (int64_t)p->n_long * a.n_heads;
        hipLaunchKernelGGL(gat_alpha_long_merge_kernel, dim3((unsigned)((pairs + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                           a.stream, p->n_long, a.n_heads, p->long_row, p->long_first, pm, pl, row_m, row_l, dead);
        SGX_LAUNCH_CHECK();
        if (a.S) {                             // the caller wants the weights themselves; otherwise stage B forms them from the scores
            hipLaunchKernelGGL(gat_alpha_long_write_kernel, dim3((p->n_tasks + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0,
                               a.stream, p->n_tasks, a.n_heads, p->task_e0, p->task_e1, pm, pl, W);
            SGX_LAUNCH_CHECK();
        }
    }
    return SGX_OK;
}

template <typename T>
int alpha_stage_heads(const sgx_gat_args &a, float *W, bool scan)
{
    if (a.n_heads % 8 == 0) return alpha_stage<T, 8>(a, W, scan);
    if (a.n_heads % 4 == 0) return alpha_stage<T, 4>(a, W, scan);
    if (a.n_heads % 2 == 0) return alpha_stage<T, 2>(a, W, scan);
    return alpha_stage<T, 1>(a, W, scan);
}

}  // namespace

int sgx_gat_alpha_stage(const sgx_gat_args &a, float *W, bool scan)
{
    return a.dtype == SGX_F16 ? alpha_stage_heads<f16>(a, W, scan) : alpha_stage_heads<float>(a, W, scan);
}
