// Entry-split CSR aggregation  D = act(A . H)  for gfx950: sgx_spmm_csr's contract in SGX_ACC_F32 arithmetic on a schedule
// that depends on the stored-entry count alone -- no plan, nothing read back, nothing allocated, the grid known from a
// capacity.  The rule ("entry-split aggregation", include/sgx.h; in numpy: tests/_spmm_flat_ref.py):
//   * the stored entries are cut into chunks of T = kFlatChunk consecutive entries, a wavefront per chunk.  Chunk c owns
//     the rows that START in [cT, (c+1)T) -- found by two searches in rowPtr, 64 probes a step -- and, where entry cT lies
//     inside a row that started earlier, that row's piece [cT, ...) (its head piece);
//   * a row wholly inside the chunk is summed and stored by it;
//   * a row that crosses a chunk end leaves one fp32 partial row per chunk it touches: the chunk it starts in (its
//     leader) in that chunk's tail slot, every later one in its head slot.  The leader also writes down the row and the
//     last chunk it reaches; the second launch, a thread per (chunk, column), adds tail + heads in chunk order and stores;
//   * an empty row starts at entry rowPtr[r] like any other and is stored as act(0) = +0 by the chunk that owns that
//     entry -- by the last live chunk when the index is the matrix's end, by chunk 0 when the matrix holds nothing.
// Every row of D is written exactly once, with plain vector stores and without atomics; the order of a row's sum depends
// on rowPtr, T and the lane split only.
// Inside a chunk a piece goes to one group of LPR lanes (LPR lanes x 16 bytes = a row of H), 64 / LPR pieces at a time,
// walked exactly as the sblock path of spmm_csr.hip walks a row (accumulate_edges: the same chain per output element, so a
// short row inside one chunk gets the bits the unplanned sgx_spmm_csr gives it).  A piece of kFlatCoop entries and more would
// leave the other groups idle for 8 steps and longer: those are taken afterwards by all groups together, 64 entries a
// step, folded with lane shuffles -- the split path's walk.
#include "spmm_device.h"
#include "flat_device.h"          // T, the piece kinds, the chunk count and the search in rowPtr

namespace {

static inline size_t flat_partial_bytes(int64_t chunks, int n_feat)
{
    return sgx_align_up((size_t)chunks * 2 * (size_t)flat_ldp(n_feat) * sizeof(float), 256);
}

// scratch: [chunks][2][ldp] fp32 partial rows (head slot, tail slot), then meta [chunks][2] = (the row the chunk leads
// or -1, the last chunk that row reaches)
template <typename T, int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void spmm_flat_kernel(
    int n_rows, int n_feat, int nnz_cap, int n_chunks, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const T *__restrict__ val, const T *__restrict__ H, unsigned h_bytes, unsigned ld_bytes, T *__restrict__ D, int64_t ldd,
    int relu, sgx_epilogue ep, float *__restrict__ partial, int ldp, int32_t *__restrict__ meta)
{
    constexpr int RPW = 64 / LPR, TILE = LPR * VEC;
    const int c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (c >= n_chunks) return;
    // the matrix's own end, read here: nnz_cap is a bound on it (and what the arrays hold, so never read past it)
    int nnz = rowptr[n_rows];
    nnz = nnz < 0 ? 0 : (nnz > nnz_cap ? nnz_cap : nnz);
    const int64_t lo64 = (int64_t)c * kFlatChunk;
    if (lo64 >= nnz && !(c == 0 && nnz == 0)) return;              // a chunk of the capacity behind the end
    const int lo = (int)lo64;
    const bool last = lo64 + kFlatChunk >= nnz;
    const int hi = last ? nnz : lo + kFlatChunk;

    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const int r_a = wave_lower_bound(rowptr, n_rows, lo);                        // the rows that start here: [r_a, r_b)
    const int r_b = last ? n_rows : wave_lower_bound(rowptr, n_rows, hi);
    const int head_end = rowptr[r_a];                                            // (r_a <= n_rows)
    const bool has_head = r_a > 0 && head_end > lo && hi > lo;                   // entry lo lies in row r_a - 1
    int tail_row = -1, tail_last = 0;
    if (!last && r_b > r_a) {
        int e = rowptr[r_b];
        e = e > nnz ? nnz : e;
        if (e > hi) { tail_row = r_b - 1; tail_last = (e - 1) / kFlatChunk; }
    }
    if (lane == 0) {
        meta[2 * (int64_t)c] = tail_row;
        meta[2 * (int64_t)c + 1] = tail_last < n_chunks ? tail_last : n_chunks - 1;
    }

    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(H), 0, h_bytes, 0x00020000);
    float *head_slot = partial + 2 * (int64_t)c * ldp;
    // a lane's VEC sums of one piece go to the row of D -- through the epilogue, the one place this launch applies it -- or,
    // raw, to the chunk's head / tail partial row
    auto emit = [&](int kind, int r, int col0, const float *acc) SGX_LAMBDA_INLINE {
        if (kind == FLAT_ROW) {
            if (col0 < n_feat) store_row<T, VEC>(D + (int64_t)r * ldd, col0, n_feat, acc, relu, ep);
        } else if (kind != FLAT_NONE) {
            float *slot = head_slot + (kind == FLAT_TAIL ? ldp : 0);
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (col0 + i < n_feat) slot[col0 + i] = acc[i];
        }
    };

    // piece 0 = the head piece (or nothing), piece i >= 1 = row r_a + i - 1
    const int64_t n_pieces = 1 + (int64_t)(r_b - r_a);
    for (int64_t i0 = 0; i0 < n_pieces; i0 += RPW) {
        const int64_t i = i0 + grp;
        int kind = FLAT_NONE, r = 0, e0 = 0, e1 = 0;
        if (i == 0) {
            if (has_head) { kind = FLAT_HEAD; r = r_a - 1; e0 = lo; e1 = head_end; }
        } else if (i < n_pieces) {
            r = r_a + (int)(i - 1);
            kind = r == tail_row ? FLAT_TAIL : FLAT_ROW;
            e0 = rowptr[r];
            e1 = rowptr[r + 1];
        }
        // (a rowPtr that is not monotone must not send a read outside the chunk)
        e0 = e0 < lo ? lo : e0;
        e1 = e1 > hi ? hi : e1;
        e1 = e1 < e0 ? e0 : e1;
        const bool coop = RPW > 1 && e1 - e0 >= kFlatCoop;
        unsigned long long coop_lanes = __ballot(coop && sub == 0);
        if (coop_lanes != ~0ull) {               // (not every group's piece is a long one)
            const int e1_own = coop ? e0 : e1;
            for (int c0 = 0; c0 < n_feat; c0 += TILE) {
                const int col0 = c0 + sub * VEC;
                const unsigned chunk_off[1] = {col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB};
                float acc[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
                accumulate_edges<T, VEC, LPR, 1, false, SGX_SPMM_ADJ_STYLE>(acc, e0, e1_own, LPR, sub, col, val, rsrc, H, ld_bytes, chunk_off);
                if (!coop) emit(kind, r, col0, acc);
            }
        }
        if constexpr (RPW > 1) {
            while (coop_lanes) {
                const int src = __ffsll(coop_lanes) - 1;
                coop_lanes &= coop_lanes - 1;
                const int ck = __shfl(kind, src), cr = __shfl(r, src), ce0 = __shfl(e0, src), ce1 = __shfl(e1, src);
                for (int c0 = 0; c0 < n_feat; c0 += TILE) {
                    const int col0 = c0 + sub * VEC;
                    const unsigned chunk_off[1] = {col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB};
                    float acc[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
                    accumulate_edges<T, VEC, LPR, 1, false, SGX_SPMM_ADJ_STYLE>(acc, ce0 + grp * LPR, ce1, 64, sub, col, val, rsrc, H, ld_bytes,
                                                                                 chunk_off);
#pragma unroll
                    for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
                        for (int k = 0; k < VEC; ++k) acc[k] += __shfl_xor(acc[k], off);
                    if (grp == 0) emit(ck, cr, col0, acc);
                }
            }
        }
    }
}

// The rows that cross a chunk end: thread (c, j) adds column j of the row chunk c leads -- its tail slot, then the head
// slots of the chunks behind it up to the last one the row reaches -- and stores it.
template <typename T>
__global__ __launch_bounds__(kBlock) void spmm_flat_finish_kernel(
    int n_rows, int n_feat, int nnz_cap, int n_chunks, const int32_t *__restrict__ rowptr, const float *__restrict__ partial, int ldp,
    const int32_t *__restrict__ meta, T *__restrict__ D, int64_t ldd, int relu, sgx_epilogue ep)
{
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (int64_t)n_chunks * n_feat) return;
    const int c = (int)(gid / n_feat), j = (int)(gid % n_feat);
    int nnz = rowptr[n_rows];
    nnz = nnz > nnz_cap ? nnz_cap : nnz;
    if ((int64_t)c * kFlatChunk >= nnz) return;                    // behind the end: the first launch left no meta there
    const int r = meta[2 * (int64_t)c];
    if (r < 0 || r >= n_rows) return;
    const int c_last = meta[2 * (int64_t)c + 1];
    const float s = sum_task_partials(partial, 2 * ldp, j, c + 1, c_last + 1, partial[(2 * (int64_t)c + 1) * ldp + j]);
    D[(int64_t)r * ldd + j] = finish_value<T>(s, relu, ep);       // the merged row's one pass through the epilogue
}

struct FlatArgs {
    int relu, n_rows, n_feat, nnz, n_chunks;
    const int32_t *rowptr, *col;
    const void *val, *H;
    unsigned h_bytes, ld_bytes;
    void *D;
    int64_t ldd;
    float *partial;
    int ldp;
    int32_t *meta;
    sgx_epilogue ep;              // on the store of a finished row (fp32 outputs; all zero = off)
    hipStream_t stream;
};

template <typename T, int VEC, int LPR>
int flat_launch(const FlatArgs &a)
{
    constexpr int kWaves = kBlock / 64;
    hipLaunchKernelGGL((spmm_flat_kernel<T, VEC, LPR>), dim3((unsigned)((a.n_chunks + kWaves - 1) / kWaves)), dim3(kBlock), 0, a.stream,
                       a.n_rows, a.n_feat, a.nnz, a.n_chunks, a.rowptr, a.col, (const T *)a.val, (const T *)a.H, a.h_bytes, a.ld_bytes,
                       (T *)a.D, a.ldd, a.relu, a.ep, a.partial, a.ldp, a.meta);
    SGX_LAUNCH_CHECK();
    const int64_t total = (int64_t)a.n_chunks * a.n_feat;
    hipLaunchKernelGGL((spmm_flat_finish_kernel<T>), dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, a.stream,
                       a.n_rows, a.n_feat, a.nnz, a.n_chunks, a.rowptr, a.partial, a.ldp, a.meta, (T *)a.D, a.ldd, a.relu, a.ep);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

}  // namespace

extern "C" int sgx_spmm_flat_chunk(void) { return kFlatChunk; }

extern "C" size_t sgx_spmm_flat_scratch_bytes(int64_t nnz, int n_feat)
{
    if (nnz < 0 || nnz > kFlatMaxNnz || n_feat < 1) return 0;
    const int64_t chunks = flat_chunks(nnz);
    return flat_partial_bytes(chunks, n_feat) + sgx_align_up((size_t)chunks * 2 * sizeof(int32_t), 256);
}

extern "C" int sgx_spmm_csr_flat(int dtype, int relu, int n_rows, int n_cols, int n_feat, int64_t nnz,
                                 const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                 const void *H, int64_t ldh, void *D, int64_t ldd,
                                 void *scratch, size_t scratch_bytes, void *stream)
{
    return sgx_spmm_csr_flat_ep(dtype, relu, n_rows, n_cols, n_feat, nnz, rowPtr, columnIndex, values, H, ldh, D, ldd, scratch,
                                scratch_bytes, /*out_scale*/0.0f, /*rq_scale_fea*/0, /*rq_internal_bits*/0, stream);
}

// The quantised layer's store epilogue on the entry-split schedule: the partial rows stay raw fp32 sums, and a finished row
// passes finish_value once -- in the chunk that holds it whole, in the cooperative walk, or in the second launch.
extern "C" int sgx_spmm_csr_flat_ep(int dtype, int relu, int n_rows, int n_cols, int n_feat, int64_t nnz,
                                    const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                    const void *H, int64_t ldh, void *D, int64_t ldd,
                                    void *scratch, size_t scratch_bytes, float out_scale, int rq_scale_fea, int rq_internal_bits,
                                    void *stream)
{
    if (n_rows < 0 || n_cols < 0 || n_feat < 1 || ldh < n_feat || ldd < n_feat || nnz < 0 || nnz > kFlatMaxNnz) return SGX_ERR_SHAPE;
    if (dtype != SGX_F16 && dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    sgx_epilogue ep = sgx_no_epilogue();
    if (rq_internal_bits != 0) {
        // the H-stage rule, with the layer's ranges (check_desc); fp32 only, as every requantising stage
        if (rq_scale_fea < 0 || rq_scale_fea > 30 || rq_internal_bits < 1 || rq_internal_bits > 30 || dtype != SGX_F32)
            return SGX_ERR_UNSUPPORTED;
        ep = sgx_requant_epilogue(rq_scale_fea, rq_internal_bits);
    }
    ep.out_scale = out_scale;
    if (n_rows == 0) return SGX_OK;
    if (!rowPtr || !D) return SGX_ERR_NULL;
    if (nnz > 0 && (!columnIndex || !values)) return SGX_ERR_NULL;
    if (nnz > 0 && n_cols > 0 && !H) return SGX_ERR_NULL;
    // the flat form is for batch-sized matrices: 32-bit buffer offsets only
    const size_t es = sgx_elem_size(dtype);
    if (sgx_spmm_table_big(dtype, n_cols, ldh, n_feat) || (unsigned long long)ldh * es >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;
    if (!scratch || scratch_bytes < sgx_spmm_flat_scratch_bytes(nnz, n_feat)) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)scratch % 256 != 0 || (uintptr_t)rowPtr % 4 != 0 || (uintptr_t)columnIndex % 4 != 0 || (uintptr_t)values % es != 0 ||
        (uintptr_t)H % es != 0 || (uintptr_t)D % es != 0)
        return SGX_ERR_ALIGN;

    FlatArgs a;
    a.relu = relu; a.n_rows = n_rows; a.n_feat = n_feat; a.nnz = (int)nnz; a.n_chunks = (int)flat_chunks(nnz);
    a.rowptr = rowPtr; a.col = columnIndex; a.val = values; a.H = H;
    a.h_bytes = (unsigned)((unsigned long long)n_cols * (unsigned long long)ldh * es); a.ld_bytes = (unsigned)(ldh * es);
    a.D = D; a.ldd = ldd; a.ep = ep; a.stream = (hipStream_t)stream;
    a.partial = (float *)scratch;
    a.ldp = flat_ldp(n_feat);
    a.meta = (int32_t *)((char *)scratch + flat_partial_bytes(a.n_chunks, n_feat));
    const sgx_lane_split split = sgx_spmm_lane_split(dtype, H, ldh, n_feat, false);
    auto run = [&](auto t, auto vec, auto lpr) { return flat_launch<decltype(t), decltype(vec)::value, decltype(lpr)::value>(a); };
    if (dtype == SGX_F16) return split.vec ? sgx_gat_dispatch_lpr<f16, 8>(split.slots, run) : sgx_gat_dispatch_lpr<f16, 1>(split.slots, run);
    return split.vec ? sgx_gat_dispatch_lpr<float, 4>(split.slots, run) : sgx_gat_dispatch_lpr<float, 1>(split.slots, run);
}
