// Entry-split GAT aggregate  D = act(softmax_row(E) . Wh)  for gfx950, one head: sgx_gat_aggregate's arithmetic on the
// schedule of sgx_spmm_csr_flat -- no plan, nothing read back, nothing allocated, the grids known from a capacity, so the call
// records into a graph and replays; balanced on any degree distribution because the work is cut by stored entries.
// The ownership rule is flat_device.h's, unchanged.  What differs from the plain form is the state of a piece: a running
// softmax state (m, l, acc[F]) in fp32 -- m the maximum of the live scores seen, l the sum of exp(E_e - m) over them, acc
// the weighted row, rescaled when m moves; a piece without a live entry is (-inf, 0, 0).
//   launch 1  a wavefront per chunk.  A piece goes to one group of LPR lanes, 64 / LPR pieces at a time, walked as
//             gat_one_pass.hip walks a row: LPR entries scored by the group's lanes, their maximum folded with shuffles, one
//             rescale, then the LPR rows gathered.  A piece of kFlatCoop entries and more is taken afterwards by all
//             groups together, 64 entries a step: the 64 scores' maximum is folded over the wavefront, so all groups keep
//             one m and their weighted rows and sums are simply added (shuffles) at the end.  A row inside the chunk is
//             normalised and stored; a crossing row's piece leaves (m, l, acc) in its slot.
//   launch 2  a thread per (chunk, column): for a leader M = max m_k, l = sum l_k exp(m_k - M), acc likewise, in chunk
//             order; the row is stored once.  A partial with m_k = -inf contributes nothing (rescale_factor), also when
//             M = -inf: that row is dead.
// Every row of D, and of row_max / row_sum, is written exactly once by plain stores; the order of every sum depends on
// rowPtr, T and the lane split only.
// The scores Wh.a1 / Wh.a2 are the aggregate's pre-pass (gat.hip) into this call's scratch; a neighbour's score is a
// 4-byte range-checked gather, E_e = LeakyReLU(fp32(s1[i] + s2[c])) as the statistics form it (gat_device.h).
#include "gat_device.h"
#include "flat_device.h"

namespace {

// where everything lies in the scratch (bytes; every region on 256)
struct gat_flat_layout {
    size_t s1, s2, slabs, mean, acc, ml, meta, total;
    int ldp;
};

gat_flat_layout flat_layout(int64_t nnz, int n_cols, int n_feat, int mean_rule)
{
    gat_flat_layout L{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t off = at; at += sgx_align_up(bytes, 256); return off; };
    const size_t chunks = (size_t)flat_chunks(nnz);
    L.ldp = flat_ldp(n_feat);
    L.s1 = take((size_t)n_cols * sizeof(float));
    L.s2 = take((size_t)n_cols * sizeof(float));
    L.slabs = take(mean_rule ? sgx_gat_mean_slab_floats(n_feat) * sizeof(float) : 0);
    L.mean = take(mean_rule ? (size_t)n_feat * sizeof(float) : 0);
    L.acc = take(chunks * 2 * (size_t)L.ldp * sizeof(float));          // [chunks][2][ldp]: head slot, tail slot
    L.ml = take(chunks * 2 * 2 * sizeof(float));                       // [chunks][2][2]: (m, l) of each slot
    L.meta = take(chunks * 2 * sizeof(int32_t));                       // [chunks][2]: (the row the chunk leads or -1, its last chunk)
    L.total = at;
    return L;
}

// What a finished element of D becomes: gat_finish (ReLU) and then the quantised layer's deq_o on fp32 outputs, as the row
// kernels' gat_finish applies it.  The kernels take the factor as `scale`, with 1 for "off" (the host maps out_scale = 0 to
// it): x * 1 is x bit for bit, and the unconditional multiply keeps the test of the factor -- a uniform branch and the
// scalar registers it pins -- out of the store path (with it the two widest fp32 instantiations spilled two SGPRs).
template <typename T>
__device__ __forceinline__ T flat_finish(float sum, int relu, float scale)
{
    T v = gat_finish<T>(sum, relu, 0.0f);
    if constexpr (sizeof(T) == 4) v = v * scale;
    return v;
}

struct gat_flat_ptrs {
    const int32_t *rowptr, *col;
    const float *s1, *s2, *fill;
    float *pacc, *pml, *row_max, *row_sum;
    int32_t *meta;
};

// Entries [e0, e1) into the state (m, l, acc): W lanes (a lane group, or the wavefront) score W entries a step -- lane wl
// of them the entry base + wl --, fold their maximum and rescale once; each group of LPR lanes then gathers the rows of
// the LPR entries its own lanes scored.  l is the lane's share of the sum.
template <typename T, int VEC, int LPR, int W>
__device__ __forceinline__ void flat_walk(float &m, float &l, float *acc, int e0, int e1, int wl, int sub, float si, float alpha,
                                          const int32_t *__restrict__ col, const T *__restrict__ val,
                                          __amdgpu_buffer_rsrc_t s2_rsrc, __amdgpu_buffer_rsrc_t rsrc, unsigned ld_bytes, unsigned col_off)
{
    constexpr int UNR = LPR < 8 ? LPR : 8;
    for (int base = e0; base < e1; base += W) {
        const int idx = base + wl;
        int c = 0;
        float x = -INFINITY;
        if (idx < e1) {
            c = col[idx];
            const float xe = leaky(si + buffer_f32(s2_rsrc, (unsigned)c * 4u), alpha);
            if (Elem<T>::to_f32(val[idx]) > 0.0f) x = xe;
        }
        float pmax = x;
#pragma unroll
        for (int off = 1; off < W; off <<= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, off));
        if (pmax == -INFINITY) continue;            // no live entry in this step (uniform across the W lanes)
        const float m_new = fmaxf(m, pmax);
        const float scale = rescale_factor(m, m_new);
        const float p = x == -INFINITY ? 0.0f : expf(x - m_new);
        m = m_new;
        l = l * scale + p;
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] *= scale;
        const int n = e1 - (base + (wl - sub));     // entries from this group's first one on
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
}

template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void gat_flat_kernel(
    int n_rows, int n_feat, int nnz_cap, int n_chunks, gat_flat_ptrs q, const T *__restrict__ val, const T *__restrict__ Wh,
    unsigned h_bytes, unsigned ld_bytes, unsigned s2_bytes, float alpha, T *__restrict__ D, int64_t ldd, int relu, float scale, int vec_store, int ldp)
{
    constexpr int RPW = 64 / LPR, TILE = LPR * VEC;
    const int c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (c >= n_chunks) return;
    flat_chunk ch;
    if (!flat_chunk_find(ch, c, n_rows, nnz_cap, n_chunks, q.rowptr, q.meta)) return;

    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Wh), 0, h_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t s2_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(q.s2), 0, s2_bytes, 0x00020000);
    // a lane's VEC columns of one piece's state (l: the whole sum): the row of D normalised, or the chunk's head / tail slot
    auto emit = [&](int kind, int r, int col0, bool first_tile, float m, float l, float *acc) SGX_LAMBDA_INLINE {
        if (kind == FLAT_ROW) {
            const bool dead = !(l > 0.0f);
            if (first_tile && sub == 0 && q.row_max) { q.row_max[r] = dead ? 0.0f : m; q.row_sum[r] = dead ? 0.0f : l; }
            if (col0 >= n_feat) return;
            const float inv_l = dead ? 0.0f : 1.0f / l;
            T out[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float v = dead ? ((q.fill && col0 + i < n_feat) ? q.fill[col0 + i] : 0.0f) : acc[i] * inv_l;
                out[i] = flat_finish<T>(v, relu, scale);
            }
            T *drow = D + (int64_t)r * ldd;
            if (VEC > 1 && vec_store && col0 + VEC <= n_feat) {
                *reinterpret_cast<u32x4 *>(drow + col0) = *reinterpret_cast<const u32x4 *>(out);
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    if (col0 + i < n_feat) drow[col0 + i] = out[i];
            }
        } else if (kind != FLAT_NONE) {
            const int64_t slot = 2 * (int64_t)c + (kind == FLAT_TAIL ? 1 : 0);
            if (first_tile && sub == 0) { q.pml[2 * slot] = m; q.pml[2 * slot + 1] = l; }
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (col0 + i < n_feat) q.pacc[slot * ldp + col0 + i] = acc[i];
        }
    };

    const int64_t n_pieces = flat_pieces(ch);
    for (int64_t i0 = 0; i0 < n_pieces; i0 += RPW) {
        int kind, r, e0, e1;
        flat_piece(ch, i0 + grp, n_pieces, q.rowptr, kind, r, e0, e1);
        const float si = kind != FLAT_NONE ? q.s1[r] : 0.0f;
        const bool coop = RPW > 1 && e1 - e0 >= kFlatCoop;
        unsigned long long coop_lanes = __ballot(coop && sub == 0);
        if (coop_lanes != ~0ull) {               // (not every group's piece is a long one)
            const int e1_own = coop ? e0 : e1;
            for (int c0 = 0; c0 < n_feat; c0 += TILE) {
                const int col0 = c0 + sub * VEC;
                const unsigned col_off = col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
                float m = -INFINITY, l = 0.0f, acc[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
                flat_walk<T, VEC, LPR, LPR>(m, l, acc, e0, e1_own, sub, sub, si, alpha, q.col, val, s2_rsrc, rsrc, ld_bytes, col_off);
#pragma unroll
                for (int off = 1; off < LPR; off <<= 1) l += __shfl_xor(l, off);
                if (!coop) emit(kind, r, col0, c0 == 0, m, l, acc);
            }
        }
        if constexpr (RPW > 1) {
            while (coop_lanes) {
                const int src = __ffsll(coop_lanes) - 1;
                coop_lanes &= coop_lanes - 1;
                const int ck = __shfl(kind, src), cr = __shfl(r, src), ce0 = __shfl(e0, src), ce1 = __shfl(e1, src);
                const float csi = __shfl(si, src);
                for (int c0 = 0; c0 < n_feat; c0 += TILE) {
                    const int col0 = c0 + sub * VEC;
                    const unsigned col_off = col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
                    float m = -INFINITY, l = 0.0f, acc[VEC];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
                    flat_walk<T, VEC, LPR, 64>(m, l, acc, ce0, ce1, lane, sub, csi, alpha, q.col, val, s2_rsrc, rsrc, ld_bytes, col_off);
                    // one m over the wavefront: the groups' sums and weighted rows are added as they are
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) l += __shfl_xor(l, off);
#pragma unroll
                    for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
                    if (grp == 0) emit(ck, cr, col0, c0 == 0, m, l, acc);
                }
            }
        }
    }
}

// The rows that cross a chunk end: thread (c, j) merges column j of the states of the row chunk c leads -- its tail slot,
// then the head slots of the chunks behind it up to the last one the row reaches -- and stores it.
template <typename T>
__global__ __launch_bounds__(kBlock) void gat_flat_finish_kernel(
    int n_rows, int n_feat, int nnz_cap, int n_chunks, gat_flat_ptrs q, int ldp, T *__restrict__ D, int64_t ldd, int relu, float scale)
{
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (int64_t)n_chunks * n_feat) return;
    const int c = (int)(gid / n_feat), j = (int)(gid % n_feat);
    int nnz = q.rowptr[n_rows];
    nnz = nnz > nnz_cap ? nnz_cap : nnz;
    if ((int64_t)c * kFlatChunk >= nnz) return;                    // behind the end: the first launch left no meta there
    const int r = q.meta[2 * (int64_t)c];
    if (r < 0 || r >= n_rows) return;
    int c_last = q.meta[2 * (int64_t)c + 1];
    c_last = c_last < n_chunks ? c_last : n_chunks - 1;
    // slot of step t: the leader's tail slot, then the head slots of chunks c + 1 .. c_last
    float M = q.pml[2 * (2 * (int64_t)c + 1)];
    for (int k = c + 1; k <= c_last; ++k) M = fmaxf(M, q.pml[2 * (2 * (int64_t)k)]);
    float l = 0.0f, a = 0.0f;
    for (int k = c; k <= c_last; ++k) {
        const int64_t slot = 2 * (int64_t)k + (k == c ? 1 : 0);
        const float w = rescale_factor(q.pml[2 * slot], M);        // (m_k = -inf: 0, also when M = -inf)
        l += q.pml[2 * slot + 1] * w;
        a += q.pacc[slot * ldp + j] * w;
    }
    const bool dead = !(l > 0.0f);
    const float out = dead ? (q.fill ? q.fill[j] : 0.0f) : a / l;
    D[(int64_t)r * ldd + j] = flat_finish<T>(out, relu, scale);
    if (j == 0 && q.row_max) { q.row_max[r] = dead ? 0.0f : M; q.row_sum[r] = dead ? 0.0f : l; }
}

struct GatFlatArgs {
    int relu, n_rows, n_cols, n_feat, nnz, n_chunks, vec_store, ldp;
    float alpha, scale;           // scale: deq_o of the quantised layer on the store of a finished row (fp32; 1 = off, see flat_finish)
    gat_flat_ptrs q;
    const void *val, *Wh;
    unsigned h_bytes, ld_bytes;
    void *D;
    int64_t ldd;
    hipStream_t stream;
};

template <typename T, int VEC, int LPR>
int gat_flat_launch(const GatFlatArgs &a)
{
    constexpr int kWaves = kBlock / 64;
    hipLaunchKernelGGL((gat_flat_kernel<T, VEC, LPR>), dim3((unsigned)((a.n_chunks + kWaves - 1) / kWaves)), dim3(kBlock), 0, a.stream,
                       a.n_rows, a.n_feat, a.nnz, a.n_chunks, a.q, (const T *)a.val, (const T *)a.Wh, a.h_bytes, a.ld_bytes,
                       (unsigned)((size_t)a.n_cols * 4), a.alpha, (T *)a.D, a.ldd, a.relu, a.scale, a.vec_store, a.ldp);
    SGX_LAUNCH_CHECK();
    const int64_t total = (int64_t)a.n_chunks * a.n_feat;
    hipLaunchKernelGGL((gat_flat_finish_kernel<T>), dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, a.stream,
                       a.n_rows, a.n_feat, a.nnz, a.n_chunks, a.q, a.ldp, (T *)a.D, a.ldd, a.relu, a.scale);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

}  // namespace

extern "C" size_t sgx_gat_flat_scratch_bytes(int64_t nnz, int n_rows, int n_cols, int n_feat, int mean_rule)
{
    if (nnz < 0 || nnz > kFlatMaxNnz || n_rows < 0 || n_cols < n_rows || n_feat < 1) return 0;
    return flat_layout(nnz, n_cols, n_feat, mean_rule != 0).total;
}

extern "C" int sgx_gat_aggregate_flat(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha, int64_t nnz,
                                      const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                      const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd,
                                      const float *fill, int64_t n_nodes, void *scratch, size_t scratch_bytes,
                                      const sgx_gat_stats *stats, void *stream)
{
    return sgx_gat_aggregate_flat_ep(dtype, relu, n_rows, n_cols, n_feat, n_heads, alpha, nnz, rowPtr, columnIndex, values, Wh, ldh,
                                     attention, D, ldd, fill, n_nodes, scratch, scratch_bytes, stats, /*out_scale*/0.0f, stream);
}

// With the quantised layer's deq_o on the store of a finished row (flat_finish: where the row kernels' gat_finish applies
// it, after the normalisation or the dead row's fill, after ReLU); the states in the slots and the statistics never see it.
extern "C" int sgx_gat_aggregate_flat_ep(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha, int64_t nnz,
                                         const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                         const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd,
                                         const float *fill, int64_t n_nodes, void *scratch, size_t scratch_bytes,
                                         const sgx_gat_stats *stats, float out_scale, void *stream)
{
    if (n_heads < 1) n_heads = 1;
    int mean_rule = 0;
    if (fill) {
        if (n_nodes < 1 || n_nodes > 0x7FFFFFFF) return SGX_ERR_SHAPE;
    } else if (n_nodes != 0) {
        if (n_nodes != n_cols) return SGX_ERR_SHAPE;
        mean_rule = 1;
    }
    if (n_rows < 0 || n_cols < n_rows || n_feat < 1 || ldh < n_feat || ldd < n_feat || nnz < 0 || nnz > kFlatMaxNnz) return SGX_ERR_SHAPE;
    if (n_heads != 1) return SGX_ERR_UNSUPPORTED;                  // one head: the reference's semantics
    if (dtype != SGX_F16 && dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    if (n_rows == 0) return SGX_OK;
    if (!rowPtr || !D || !Wh || !attention) return SGX_ERR_NULL;
    if (nnz > 0 && (!columnIndex || !values)) return SGX_ERR_NULL;
    if (stats) {
        const int rc = sgx_gat_stats_check(stats, n_cols, 1);
        if (rc != SGX_OK) return rc;
    }
    // the flat form is for batch-sized matrices: 32-bit buffer offsets only
    const size_t es = sgx_elem_size(dtype);
    const unsigned long long table_bytes = (unsigned long long)n_cols * (unsigned long long)ldh * es;
    if (sgx_spmm_table_big(dtype, n_cols, ldh, n_feat) || (unsigned long long)ldh * es >= 0xFFFFFFF0ull || table_bytes >= 0xFFFFFFF0ull ||
        (unsigned long long)n_cols * 4ull >= 0xFFFFFFF0ull)
        return SGX_ERR_UNSUPPORTED;
    const gat_flat_layout L = flat_layout(nnz, n_cols, n_feat, mean_rule);
    if (!scratch || scratch_bytes < L.total) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)scratch % 256 != 0 || (uintptr_t)rowPtr % 4 != 0 || (uintptr_t)columnIndex % 4 != 0 || (uintptr_t)values % es != 0 ||
        (uintptr_t)Wh % es != 0 || (uintptr_t)attention % es != 0 || (uintptr_t)D % es != 0 || (uintptr_t)fill % 4 != 0)
        return SGX_ERR_ALIGN;

    char *base = (char *)scratch;
    hipStream_t s = (hipStream_t)stream;
    // the aggregate's pre-pass on this call's scratch: s1 at float offset 0, s2 behind it
    sgx_gat_args g{};
    g.dtype = dtype; g.relu = relu; g.n_rows = n_rows; g.n_cols = n_cols; g.n_feat = n_feat; g.n_heads = 1; g.alpha = alpha;
    g.rowptr = rowPtr; g.col = columnIndex; g.val = values; g.Wh = Wh; g.att = attention; g.ldh = ldh; g.ldd = ldd;
    g.h_bytes = (unsigned)table_bytes; g.ld_bytes = (unsigned)(ldh * es); g.D = D; g.stream = s;
    g.scratch = (float *)base;
    g.lay.s1 = L.s1 / sizeof(float); g.lay.s2 = L.s2 / sizeof(float);
    sgx_gat_lane_split(g);
    int rc = sgx_gat_scores_launch(g);
    if (rc != SGX_OK) return rc;
    const float *fill_row = fill;
    if (mean_rule) {
        rc = sgx_gat_mean_row(dtype, n_cols, n_feat, Wh, ldh, (float *)(base + L.slabs), (float *)(base + L.mean), s);
        if (rc != SGX_OK) return rc;
        fill_row = (const float *)(base + L.mean);
    }
    if (stats) {
        SGX_HIP_CHECK(hipMemcpyAsync(stats->score_row, base + L.s1, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToDevice, s));
        SGX_HIP_CHECK(hipMemcpyAsync(stats->score_col, base + L.s2, (size_t)n_cols * sizeof(float), hipMemcpyDeviceToDevice, s));
    }

    GatFlatArgs a;
    a.relu = relu; a.n_rows = n_rows; a.n_cols = n_cols; a.n_feat = n_feat; a.nnz = (int)nnz; a.n_chunks = (int)flat_chunks(nnz);
    a.vec_store = g.vec_store; a.ldp = L.ldp; a.alpha = alpha; a.scale = out_scale != 0.0f ? out_scale : 1.0f;
    a.q.rowptr = rowPtr; a.q.col = columnIndex; a.q.s1 = (const float *)(base + L.s1); a.q.s2 = (const float *)(base + L.s2);
    a.q.fill = fill_row; a.q.pacc = (float *)(base + L.acc); a.q.pml = (float *)(base + L.ml); a.q.meta = (int32_t *)(base + L.meta);
    a.q.row_max = stats ? stats->row_max : nullptr; a.q.row_sum = stats ? stats->row_sum : nullptr;
    a.val = values; a.Wh = Wh; a.h_bytes = g.h_bytes; a.ld_bytes = g.ld_bytes; a.D = D; a.ldd = ldd; a.stream = s;
    return sgx_gat_dispatch(g, [&](auto t, auto vec, auto lpr) {
        return gat_flat_launch<decltype(t), decltype(vec)::value, decltype(lpr)::value>(a);
    });
}
