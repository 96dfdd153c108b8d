// CSR aggregation  D = act(A . H)  for gfx950 -- the A.H stage of the reference
// (loop_adj / compute2 / dsp_kernel_wrapper_adj / writec: K.cpp:3339, :2483, :1778, :713)
// and, with H := W, the sparse-feature X.W stage (compute1 in gemm_mode 0, K.cpp:1960-2078).
//
// Mapping to the hardware (HBM-bound: ~2*F flops per 6+2F bytes):
//   * sblock path.  A wavefront is cut into groups of LPR lanes; LPR lanes x 16 bytes cover
//     one row of H (F=64 fp16 -> 8 lanes, one 128-byte line).  Each group owns ONE row of A,
//     so a wavefront works on 64/LPR rows at once -- the reference's SPMM_BLOCK row grouping
//     (K.cpp:826-845) with the running-nnz interval test replaced by lane ownership.  Per
//     step a group reads LPR (column, value) pairs with one coalesced load each, broadcasts
//     them with lane shuffles, and issues LPR independent 16-byte gathers (buffer loads: an
//     edge past the end of the row gets an out-of-range offset, which returns 0 without
//     touching memory), i.e. 64 gathers of 16 bytes in flight per wavefront.
//   * split path.  Rows longer than plan->long_threshold are cut into chunks; one wavefront
//     sums one chunk with all 64/LPR groups on the same row, the groups are folded with
//     lane shuffles, the fp32 partial rows are added in chunk order by a small second kernel.
//   * products and sums in fp32, one rounding to the storage type; ReLU fused into the store.
// (the lane split, the walk over a run of entries -- accumulate_edges -- and the row store are spmm_device.h's, shared
// with the entry-split form of spmm_flat.hip)
#include "spmm_device.h"

// Tuning knob of the sblock kernel (default = the measured best, tools/sweep_spmm.py; the others: spmm_device.h):
#ifndef SGX_SPMM_MINWAVES
#define SGX_SPMM_MINWAVES 1          // 2nd __launch_bounds__ argument: min wavefronts per SIMD
#endif
#include <stdlib.h>

namespace {

constexpr double kShortRowDegree = 5.0;      // choose_cpl: mean degree below which lane groups are halved

// ---------------------------------------------------------------------------------------
// One-step rows, 64 per wavefront.  In a power-law graph most rows hold a handful of edges (R-MAT S-100M: 47 % of the
// rows are their self loop, 80 % hold at most 8 edges) and their cost is not bytes but the chain row id -> row pointers
// -> (column, value) -> gather -> store, a memory round trip per link, paid by a wavefront for 64 / LPR rows at a
// time.  Here every link of the chain is ONE round trip for 64 rows: lane l reads the row id and the row pointers of
// row l, the (column, value) pairs of all LPR iterations are requested back to back, then the lane groups take
// 64 / LPR rows per iteration as in the sblock path -- the same fma chain per output element, hence the same bits.
// The plan's degree order ends with these rows (row_order[n_multi, n_rows): at most 8 edges each).
// ---------------------------------------------------------------------------------------
template <typename T, int VEC, int LPR>
__device__ __forceinline__ void spmm_short_rows(
    const sgx_tail_tile &tile, int n_feat, const int32_t *__restrict__ col, const T *__restrict__ val, __amdgpu_buffer_rsrc_t rsrc,
    unsigned ld_bytes, T *__restrict__ D, int64_t ldd, int relu, const float *__restrict__ acc_in, float *__restrict__ acc_out,
    int64_t ld_acc, const sgx_epilogue &ep)
{
    static_assert(LPR >= 8, "a row's 8 edge slots are loaded by 8 lanes of its group");
    constexpr int RPW = 64 / LPR, ITER = LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const int r = tile.r, e0 = tile.e0, deg = tile.deg;
    const bool valid = tile.valid;
    // the (column, value) pairs of all iterations; unconditional loads (a conditional load makes hipcc wait for it at
    // the join): slots past the end of a row read entry 0 and are masked when they are used
    // (the iterations are taken 8 at a time -- the pairs of one batch are 16 registers -- whatever the lane split)
    constexpr int CH = 8;
    const int col0 = sub * VEC;
    const unsigned chunk_off = col0 < n_feat ? (unsigned)col0 * (unsigned)sizeof(T) : kOOB;
    for (int it0 = 0; it0 < ITER; it0 += CH) {
    unsigned c[CH];
    T a[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int s = (it0 + i) * RPW + grp;
        const int se0 = __shfl(e0, s), sdeg = __shfl(deg, s);
        const int e = sub < sdeg ? se0 + sub : 0;
        c[i] = (unsigned)__builtin_nontemporal_load(col + e);
        a[i] = __builtin_nontemporal_load(val + e);
    }
#pragma unroll
    for (int it = 0; it < CH; ++it) {
        const int s = (it0 + it) * RPW + grp;
        const int sdeg = __shfl(deg, s);
        const int64_t rr = __shfl(r, s);
        const bool live = __shfl((int)valid, s) != 0;
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
        if (acc_in && live) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (col0 + i < n_feat) acc[i] = acc_in[rr * ld_acc + col0 + i];
        }
        const float af = Elem<T>::to_f32(a[it]);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const unsigned cc = (unsigned)__shfl((int)c[it], t, LPR);
            const float aa = __shfl(af, t, LPR);
            Gather<T, VEC>::run(acc, aa, rsrc, (t < sdeg && chunk_off != kOOB) ? cc * ld_bytes + chunk_off : kOOB);
        }
        if (live && acc_out) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (col0 + i < n_feat) acc_out[rr * ld_acc + col0 + i] = acc[i];
        } else if (live && col0 < n_feat) {
            store_row<T, VEC>(D + rr * ldd, col0, n_feat, acc, relu, ep);
        }
    }
    }
}

// ---------------------------------------------------------------------------------------
// One launch, two kinds of workgroup.  Workgroups [0, split_blocks) run the split path: one
// wavefront per (long row, 512-edge chunk), all 64/LPR lane groups on the same row, fp32 partial
// rows.  The others run the sblock path: one group of LPR lanes per row, 64/LPR rows per
// wavefront.  Putting both in one grid lets the heavy chunks start first and the short rows fill
// in around them (on R-MAT the two paths as separate launches took 0.98 + 1.24 ms back to back).
// ---------------------------------------------------------------------------------------
template <typename T, int VEC, int LPR, int CPL, bool BIG, int STYLE, bool SHORT>
__device__ __forceinline__ void spmm_body(
    int n_rows, int n_feat, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const T *__restrict__ val, const T *__restrict__ H, unsigned h_bytes, unsigned ld_bytes,
    T *__restrict__ D, int64_t ldd, int relu, int long_threshold, int vec_store,
    const int32_t *__restrict__ row_order,
    int split_blocks, int n_tasks, const int32_t *__restrict__ task_e0, const int32_t *__restrict__ task_e1,
    float *__restrict__ partial, int ldp,
    const float *__restrict__ acc_in, float *__restrict__ acc_out, int64_t ld_acc, sgx_epilogue ep, int n_multi, int short_first)
{
    constexpr int LANE_COLS = CPL * VEC;          // columns per lane
    constexpr int TILE = LPR * LANE_COLS;         // columns covered per pass
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(H), 0, h_bytes, 0x00020000);

    if ((int)blockIdx.x < split_blocks) {
        // ---- split path ----
        const sgx_task t = schedule_task(n_tasks, task_e0, task_e1);
        if (t.index < 0) return;
        const int task = t.index, e0 = t.e0, e1 = t.e1;
        for (int c0 = 0; c0 < n_feat; c0 += TILE) {
            const int col0 = c0 + sub * LANE_COLS;
            unsigned chunk_off[CPL];
            float acc[LANE_COLS];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
                chunk_off[j] = col0 + j * VEC < n_feat ? (unsigned)(col0 + j * VEC) * (unsigned)sizeof(T) : kOOB;
#pragma unroll
            for (int i = 0; i < LANE_COLS; ++i) acc[i] = 0.0f;
            accumulate_edges<T, VEC, LPR, CPL, BIG, STYLE>(acc, e0 + grp * LPR, e1, 64, sub, col, val, rsrc, H, ld_bytes,
                                                    chunk_off);
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
                for (int i = 0; i < LANE_COLS; ++i) acc[i] += __shfl_xor(acc[i], off);
            if (grp == 0) {
#pragma unroll
                for (int i = 0; i < LANE_COLS; ++i)
                    if (col0 + i < n_feat) partial[(int64_t)task * ldp + col0 + i] = acc[i];
            }
        }
        return;
    }

    constexpr bool TAIL = SHORT && LPR >= 8 && CPL == 1 && !BIG;
    if constexpr (TAIL) {
        // ---- one-step rows: the tail of the degree order, 64 rows per wavefront ----
        if ((int)blockIdx.x >= short_first) {
            sgx_tail_tile tile;
            if (schedule_tail_tile(short_first, n_multi, n_rows, row_order, rowptr, tile))
                spmm_short_rows<T, VEC, LPR>(tile, n_feat, col, val, rsrc, ld_bytes, D, ldd, relu, acc_in, acc_out, ld_acc, ep);
            return;
        }
    }
    // ---- sblock path: n_rows = number of work items, n_multi of them ahead of a tail ----
    const int n_walk = TAIL ? n_multi : n_rows;
    int64_t r0, r_step;
    schedule_row_range<LPR, SHORT>(split_blocks, short_first, r0, r_step);
    for (; r0 < n_walk; r0 += r_step) {
        int64_t r; int e0, e1;
        const bool live = schedule_row<LPR>(r0, n_walk, long_threshold, row_order, rowptr, r, e0, e1);
        for (int c0 = 0; c0 < n_feat; c0 += TILE) {
            const int col0 = c0 + sub * LANE_COLS;
            unsigned chunk_off[CPL];
            float acc[LANE_COLS];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
                chunk_off[j] = col0 + j * VEC < n_feat ? (unsigned)(col0 + j * VEC) * (unsigned)sizeof(T) : kOOB;
#pragma unroll
            for (int i = 0; i < LANE_COLS; ++i) acc[i] = 0.0f;
            // two-pass aggregation (own-partition edges while the halo rows travel, then the halo
            // edges): the second pass starts from the first pass's fp32 sums
            if (acc_in && live) {
#pragma unroll
                for (int i = 0; i < LANE_COLS; ++i)
                    if (col0 + i < n_feat) acc[i] = acc_in[r * ld_acc + col0 + i];
            }
            accumulate_edges<T, VEC, LPR, CPL, BIG, STYLE>(acc, e0, e1, LPR, sub, col, val, rsrc, H, ld_bytes, chunk_off);
            if (live && acc_out) {
#pragma unroll
                for (int i = 0; i < LANE_COLS; ++i)
                    if (col0 + i < n_feat) acc_out[r * ld_acc + col0 + i] = acc[i];
            } else if (live) {
#pragma unroll
                for (int j = 0; j < CPL; ++j)
                    if (col0 + j * VEC < n_feat) store_row<T, VEC>(D + r * ldd, col0 + j * VEC, n_feat, acc + j * VEC, relu, ep);
            }
        }
    }
}

#define SGX_SPMM_PARAMS                                                                                           \
    int n_rows, int n_feat, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,                \
        const T *__restrict__ val, const T *__restrict__ H, unsigned h_bytes, unsigned ld_bytes, T *__restrict__ D, \
        int64_t ldd, int relu, int long_threshold, int vec_store, const int32_t *__restrict__ row_order,          \
        int split_blocks, int n_tasks, const int32_t *__restrict__ task_e0, const int32_t *__restrict__ task_e1,  \
        float *__restrict__ partial, int ldp, const float *__restrict__ acc_in, float *__restrict__ acc_out,       \
        int64_t ld_acc, sgx_epilogue ep, int n_multi, int short_first
#define SGX_SPMM_ARGS                                                                                            \
    n_rows, n_feat, rowptr, col, val, H, h_bytes, ld_bytes, D, ldd, relu, long_threshold, vec_store, row_order,  \
        split_blocks, n_tasks, task_e0, task_e1, partial, ldp, acc_in, acc_out, ld_acc, ep, n_multi, short_first

// Two entry points over the one body, so that a profile tells the stages apart:
// spmm_kernel = the A.H aggregation (loop_adj), xw_sparse_kernel = X.W with a CSR X (loop_fea, the
// weight matrix as the gathered table).
template <typename T, int VEC, int LPR, int CPL, bool BIG>
__global__ __launch_bounds__(kBlock, SGX_SPMM_MINWAVES) void spmm_kernel(SGX_SPMM_PARAMS)
{
    spmm_body<T, VEC, LPR, CPL, BIG, SGX_SPMM_ADJ_STYLE, false>(SGX_SPMM_ARGS);
}

// the A.H aggregation under a degree-ordered plan whose order ends in one-step rows: those 64 to a wavefront
// (spmm_short_rows); its own kernel so that the plain one -- the uniform graph's -- keeps its code as measured
template <typename T, int VEC, int LPR, int CPL, bool BIG>
__global__ __launch_bounds__(kBlock, SGX_SPMM_MINWAVES) void spmm_short_tail_kernel(SGX_SPMM_PARAMS)
{
    spmm_body<T, VEC, LPR, CPL, BIG, SGX_SPMM_ADJ_STYLE, true>(SGX_SPMM_ARGS);
}

template <typename T, int VEC, int LPR, int CPL, bool BIG>
__global__ __launch_bounds__(kBlock, SGX_SPMM_MINWAVES) void xw_sparse_kernel(SGX_SPMM_PARAMS)
{
    spmm_body<T, VEC, LPR, CPL, BIG, SGX_SPMM_FEA_STYLE, false>(SGX_SPMM_ARGS);
}

// ---------------------------------------------------------------------------------------
// The aggregation of a square dense fp16 layer (64 -> 64) with W applied in its epilogue:  D = act(f16(A.X) . W).
// (A.X).W gathers the same 64 columns per edge as A.(X.W) and applies W once per output row, so H = X.W is never
// written or read.  A wavefront sums 16 consecutive rows of Z = A.X, 8 at a time exactly as the sblock path does (the same
// fma chain per element), rounds them to fp16 -- the rounding the two-launch aggregate-first order applies when it stores Z
// -- into its own LDS slab, and multiplies the 16 x 64 tile by W on the matrix cores in the orientation, the fragment
// layout and the K order of xw_dense.hip's fp16 arm (D^T tile = Wt rows x Z rows, k = 32 s + 8 (lane >> 4) + j, two K
// steps from a zero accumulator, tiles paired so that a lane ends up with 8 consecutive columns): the bits of
// spmm_kernel into Z followed by sgx_xw_dense_ep.  W's fragments are staged in LDS once per workgroup; the result goes
// back through the slab so that D leaves as whole 128-byte rows from 8 consecutive lanes, the way store_row writes them.
// Slab rows lie 144 bytes apart: the 16-byte fragment reads of 16 consecutive rows then fall into disjoint banks.
// ---------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16x8 f16x8_u __attribute__((aligned(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDenseF = 64;                      // M_fea = P_w: one 128-byte row per 8 lanes, 2 K steps, 4 column tiles
constexpr int kDenseTile = 16;                   // rows of Z per MFMA tile = two 8-row groups of the wavefront
constexpr int kDensePitch = kDenseF + 8;         // halves between slab rows
#ifndef SGX_SPMM_DENSE_BLOCKS_PER_CU
#define SGX_SPMM_DENSE_BLOCKS_PER_CU 256         // grid cap (64 rows per workgroup); tiles beyond it are grid-strided
#endif                                           // S-100M layer 2, one run each: 4.688 ms per step at 256, 4.699 at 64, 4.707 at 16

// the lanes of a wavefront hand rows to one another through its slab: LDS operations of one wavefront complete in
// order, the fences keep the compiler from moving them across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kBlock, SGX_SPMM_MINWAVES) void spmm_dense_f16_kernel(
    int n_rows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const f16 *__restrict__ val,
    const f16 *__restrict__ X, unsigned x_bytes, const f16 *__restrict__ Wt, f16 *__restrict__ D, int relu)
{
    constexpr int VEC = 8, LPR = 8, RPW = 64 / LPR, KS = kDenseF / 32, NT = kDenseF / 16;
    __shared__ __attribute__((aligned(16))) f16x8 sW[KS][NT][64];                          // 8 KB, fragment layout
    __shared__ __attribute__((aligned(16))) f16 sZ[kBlock / 64][kDenseTile * kDensePitch];  // 2304 bytes per wavefront
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const int l15 = lane & 15, lq = lane >> 4;

    // MFMA row i of column tile nt stands for output column 32 (nt / 2) + 8 (i / 4) + 4 (nt % 2) + i % 4 (the pairing of
    // xw_dense_stationary_f16_kernel); lane ln of fragment (s, nt) holds k = 32 s + 8 (ln >> 4) .. + 7 of that row of Wt
    for (int i = threadIdx.x; i < KS * NT * 64; i += kBlock) {
        const int ln = i & 63, nt = (i >> 6) % NT, s = i / (64 * NT);
        const int n = (nt / 2) * 32 + 8 * ((ln & 15) / 4) + 4 * (nt % 2) + (ln & 15) % 4;
        sW[s][nt][ln] = *reinterpret_cast<const f16x8_u *>(Wt + n * kDenseF + s * 32 + 8 * (ln >> 4));
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16 *>(X), 0, x_bytes, 0x00020000);
    const unsigned chunk_off[1] = {(unsigned)(sub * VEC) * (unsigned)sizeof(f16)};
    f16 *slab = sZ[threadIdx.x >> 6];
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t r0 = wave * kDenseTile; r0 < n_rows; r0 += n_waves * kDenseTile) {
        // ---- Z: two groups of 8 rows, a row past the end (a tail's upper rows) sums nothing and leaves zeros ----
#pragma unroll 1
        for (int h = 0; h < kDenseTile / RPW; ++h) {
            const int64_t r = r0 + h * RPW + grp;
            int e0 = 0, e1 = 0;
            if (r < n_rows) {
                e0 = rowptr[r];
                e1 = rowptr[r + 1];
            }
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
            accumulate_edges<f16, VEC, LPR, 1, false, SGX_SPMM_ADJ_STYLE>(acc, e0, e1, LPR, sub, col, val, rsrc, X,
                                                                          kDenseF * (unsigned)sizeof(f16), chunk_off);
            f16x8 z;
#pragma unroll
            for (int i = 0; i < VEC; ++i) z[i] = (f16)acc[i];
            *reinterpret_cast<f16x8 *>(slab + (h * RPW + grp) * kDensePitch + sub * VEC) = z;
        }
        wave_lds_sync();
        // ---- D^T tile = Wt rows x Z rows ----
        f32x4 d[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) d[nt] = (f32x4){0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const f16x8 b = *reinterpret_cast<const f16x8 *>(slab + l15 * kDensePitch + s * 32 + 8 * lq);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) d[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sW[s][nt][lane], b, d[nt], 0, 0, 0);
        }
        wave_lds_sync();                         // every lane holds its fragments of Z: the slab takes the result
        // lane (l15, lq) holds columns 32 q + 8 lq .. + 7 of row l15; the ReLU on the rounded value as xw_dense applies it
#pragma unroll
        for (int q = 0; q < NT / 2; ++q) {
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f16 lo = (f16)d[2 * q][j], hi = (f16)d[2 * q + 1][j];
                o[j] = (!relu || lo > (f16)0) ? lo : (f16)0;
                o[4 + j] = (!relu || hi > (f16)0) ? hi : (f16)0;
            }
            *reinterpret_cast<f16x8 *>(slab + l15 * kDensePitch + q * 32 + 8 * lq) = o;
        }
        wave_lds_sync();
        // ---- rows of D: 8 lanes x 16 bytes = one 128-byte line each ----
#pragma unroll
        for (int h = 0; h < kDenseTile / RPW; ++h) {
            const int64_t r = r0 + h * RPW + grp;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(slab + (h * RPW + grp) * kDensePitch + sub * VEC);
            if (r < n_rows) *reinterpret_cast<Elem<f16>::vec16_u *>(D + r * kDenseF + sub * VEC) = v;
        }
        wave_lds_sync();                         // before the next tile's Z lands in the slab
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void spmm_split_finalize_kernel(
    int n_long, int n_feat, const int32_t *__restrict__ long_row, const int32_t *__restrict__ long_first,
    const float *__restrict__ partial, int ldp, T *__restrict__ D, int64_t ldd, int relu,
    const float *__restrict__ acc_in, float *__restrict__ acc_out, int64_t ld_acc, sgx_epilogue ep)
{
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t total = (int64_t)n_long * n_feat;
    if (gid >= total) return;
    const int l = (int)(gid / n_feat), j = (int)(gid % n_feat);
    const int64_t row = long_row[l];
    const float s = sum_task_partials(partial, ldp, j, long_first[l], long_first[l + 1], acc_in ? acc_in[row * ld_acc + j] : 0.0f);
    if (acc_out) { acc_out[row * ld_acc + j] = s; return; }
    D[row * ldd + j] = finish_value<T>(s, relu, ep);
}

// ---------------------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------------------
struct LaunchArgs {
    int relu, n_rows, n_feat;
    const int32_t *rowptr, *col;
    const void *val, *H;
    unsigned h_bytes, ld_bytes;
    void *D;
    int64_t ldd;
    const sgx_plan *plan;
    float *partial;
    int ldp;
    int vec_store;
    bool big;
    const float *acc_in;
    float *acc_out;
    int64_t ld_acc;
    bool fea_stage;           // launched for X.W (sgx_xw_sparse): same body under its own kernel name
    sgx_epilogue ep;
    hipStream_t stream;
};

template <typename T, int VEC, int LPR, int CPL, bool BIG>
int launch_one_impl(const LaunchArgs &a)
{
    const sgx_plan *p = a.plan;
    const sgx_row_schedule s = sgx_schedule_rows(p, a.n_rows, LPR, LPR * VEC, a.n_feat, !a.fea_stage && CPL == 1 && !BIG);
    if (s.grid > 0) {
        auto kernel = a.fea_stage ? xw_sparse_kernel<T, VEC, LPR, CPL, BIG>
                                  : (s.short_tail ? spmm_short_tail_kernel<T, VEC, LPR, CPL, BIG> : spmm_kernel<T, VEC, LPR, CPL, BIG>);
        hipLaunchKernelGGL(kernel, dim3(s.grid), dim3(kBlock), 0, a.stream, s.n_work, a.n_feat, a.rowptr, a.col, (const T *)a.val,
                           (const T *)a.H, a.h_bytes, a.ld_bytes, (T *)a.D, a.ldd, a.relu, s.long_threshold, a.vec_store, s.order,
                           s.split_blocks, s.n_tasks, s.task_e0, s.task_e1, a.partial, a.ldp, a.acc_in, a.acc_out, a.ld_acc, a.ep,
                           s.n_multi, s.short_first);
        SGX_LAUNCH_CHECK();
    }
    if (s.n_tasks > 0) {
        const int64_t total = (int64_t)p->n_long * a.n_feat;
        hipLaunchKernelGGL((spmm_split_finalize_kernel<T>), dim3((unsigned)((total + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, a.stream, p->n_long, a.n_feat, p->long_row, p->long_first, a.partial,
                           a.ldp, (T *)a.D, a.ldd, a.relu, a.acc_in, a.acc_out, a.ld_acc, a.ep);
        SGX_LAUNCH_CHECK();
    }
    return SGX_OK;
}

// slots = LPR * CPL = 16-byte chunks per row (power of two); cpl in {1, 2, 4}, cpl <= slots.
// Tables of 4 GiB and more always run with CPL = 1.
template <typename T, int VEC, int SLOTS>
int launch_slots(const LaunchArgs &a, int cpl)
{
    if (a.big) return launch_one_impl<T, VEC, SLOTS, 1, true>(a);
    if constexpr (VEC > 1 && SLOTS >= 4) {
        if (cpl == 4) return launch_one_impl<T, VEC, SLOTS / 4, 4, false>(a);
    }
    if constexpr (VEC > 1 && SLOTS >= 2) {
        if (cpl >= 2) return launch_one_impl<T, VEC, SLOTS / 2, 2, false>(a);
    }
    return launch_one_impl<T, VEC, SLOTS, 1, false>(a);
}

template <typename T, int VEC>
int launch_lpr(const LaunchArgs &a, int slots, int cpl)
{
    switch (slots) {
    case 1: return launch_slots<T, VEC, 1>(a, cpl);
    case 2: return launch_slots<T, VEC, 2>(a, cpl);
    case 4: return launch_slots<T, VEC, 4>(a, cpl);
    case 8: return launch_slots<T, VEC, 8>(a, cpl);
    case 16: return launch_slots<T, VEC, 16>(a, cpl);
    case 32: return launch_slots<T, VEC, 32>(a, cpl);
    default: return launch_slots<T, VEC, 64>(a, cpl);
    }
}

// Lanes per row from the mean degree.  Measured on 4 M-row uniform graphs at F = 64 fp16
// (tools/cpl_probe.py): halving the lane group (CPL = 2) wins only below ~5 edges per row
// (0.34 vs 0.47 ms at 2 edges/row, 0.48 vs 0.55 ms at 4) and loses above (1.23 vs 1.13 ms at 13,
// 2.52 vs 2.18 ms at 25; sparse X.W 0.98 vs 0.86 ms); CPL = 4 never wins.
int choose_cpl(const sgx_plan *plan, int slots)
{
    if (sgx_tune().spmm_cpl) return sgx_tune().spmm_cpl;                // tuning override (tools/cpl_probe.py)
    if (!plan || plan->n_rows <= 0 || slots < 2) return 1;
    const double avg = (double)plan->nnz / (double)plan->n_rows;
    return avg < kShortRowDegree ? 2 : 1;
}

}  // namespace

size_t sgx_spmm_scratch_bytes(const sgx_plan *plan, int n_feat)
{
    if (!plan || plan->n_tasks == 0 || n_feat <= 0) return 0;
    return sgx_align_up((size_t)plan->n_tasks * (size_t)sgx_align_up((size_t)n_feat, 4) * sizeof(float), 256);
}

// 32-bit buffer offsets need the whole table below kOOBRow and a row below 1 MiB (sgx_device.h)
bool sgx_spmm_table_big(int dtype, int n_cols, int64_t ldh, int n_feat)
{
    const size_t es = sgx_elem_size(dtype);
    return (unsigned long long)n_cols * (unsigned long long)ldh * es > kOOBRow || (unsigned long long)n_feat * es > kMaxRowBytes;
}

// The fused form walks the rows in natural order with one lane group per row: a plan that cuts rows into tasks or lists
// them in degree order (with or without a one-step tail) keeps the staged path, and so does a table past 32-bit buffer
// offsets.  16-byte gathers and fragment loads: X on a dword, Wt and D on an element (any fp16 pointer).
// (Below 5 entries per row the staged aggregation halves its lane groups, choose_cpl; this form keeps 8 lanes per row
// there -- it loses less by that than the dense pass it saves: 0.34 vs 0.47 ms at 2 entries per row on 4 M rows.)
bool sgx_spmm_dense_applicable(int n_cols, const void *X, const void *Wt, const void *D, const sgx_plan *plan)
{
    if (plan && (plan->n_tasks > 0 || plan->row_order)) return false;
    if (sgx_spmm_table_big(SGX_F16, n_cols, kDenseF, kDenseF)) return false;
    return (uintptr_t)X % 4 == 0 && (uintptr_t)Wt % 2 == 0 && (uintptr_t)D % 2 == 0;
}

int sgx_spmm_dense(int relu, int n_rows, int n_cols, const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                   const void *X, const void *Wt, void *D, hipStream_t stream)
{
    if (n_rows < 0 || n_cols < 0) return SGX_ERR_SHAPE;
    if (n_rows == 0) return SGX_OK;
    if (!rowPtr || !Wt || !D) return SGX_ERR_NULL;
    if (n_cols > 0 && (!X || !columnIndex || !values)) return SGX_ERR_NULL;
    if (!sgx_spmm_dense_applicable(n_cols, X, Wt, D, nullptr)) return SGX_ERR_UNSUPPORTED;
    const int64_t rows_per_block = (int64_t)kDenseTile * (kBlock / 64);
    int64_t blocks = ((int64_t)n_rows + rows_per_block - 1) / rows_per_block;
    const int per_cu = sgx_tune().spmm_fused_blocks_per_cu > 0 ? sgx_tune().spmm_fused_blocks_per_cu : SGX_SPMM_DENSE_BLOCKS_PER_CU;
    if (blocks > (int64_t)256 * per_cu) blocks = (int64_t)256 * per_cu;
    hipLaunchKernelGGL(spmm_dense_f16_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, n_rows, rowPtr, columnIndex,
                       (const f16 *)values, (const f16 *)X, (unsigned)((size_t)n_cols * kDenseF * sizeof(f16)), (const f16 *)Wt,
                       (f16 *)D, relu);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

int sgx_spmm_launch(int dtype, int acc_mode, int spmm_block, int relu, int n_rows, int n_cols, int n_feat,
                    const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                    const void *H, int64_t ldh, void *D, int64_t ldd,
                    const sgx_plan *plan, void *scratch, size_t scratch_bytes, hipStream_t stream,
                    const float *acc_in, float *acc_out, int64_t ld_acc, bool fea_stage, int ref_threads, sgx_epilogue ep)
{
    (void)spmm_block;
    if (n_rows < 0 || n_cols < 0 || n_feat < 1 || ldh < n_feat) return SGX_ERR_SHAPE;
    if (n_rows == 0) return SGX_OK;
    if (!rowPtr || (!D && !acc_out)) return SGX_ERR_NULL;
    if (D && ldd < n_feat) return SGX_ERR_SHAPE;
    if ((acc_in || acc_out) && (ld_acc < n_feat || acc_mode != SGX_ACC_F32)) return SGX_ERR_SHAPE;
    if (dtype != SGX_F16 && dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    if (acc_mode == SGX_ACC_REF_HALF) {
        if (dtype != SGX_F16) return SGX_ERR_UNSUPPORTED;
        if (n_cols > 0 && (!H || !columnIndex || !values)) return SGX_ERR_NULL;
        return sgx_refhalf_csr(spmm_block, ref_threads, relu, n_rows, n_cols, n_feat, rowPtr, columnIndex, values, H, ldh, D, ldd, stream);
    }
    if (acc_mode != SGX_ACC_F32) return SGX_ERR_UNSUPPORTED;
    if (plan && plan->n_rows != n_rows) return SGX_ERR_SHAPE;
    const size_t es = sgx_elem_size(dtype);
    const unsigned long long table_bytes = (unsigned long long)n_cols * (unsigned long long)ldh * es;
    const bool big = sgx_spmm_table_big(dtype, n_cols, ldh, n_feat);
    if ((unsigned long long)ldh * es >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;
    if (n_cols > 0 && (!H || !columnIndex || !values)) return SGX_ERR_NULL;
    // X.W over a large CSR X: the weight slice resident in LDS instead of gathered through L2 (same sums, same order)
    if (fea_stage && !acc_in && !acc_out && !big && sgx_xw_sparse_lds_applicable(dtype, n_rows, n_cols, n_feat, ldd, plan))
        return sgx_xw_sparse_lds(dtype, n_rows, n_cols, n_feat, rowPtr, columnIndex, values, H, ldh, D, ldd, plan, ep, stream);

    LaunchArgs a;
    a.relu = relu; a.n_rows = n_rows; a.n_feat = n_feat;
    a.rowptr = rowPtr; a.col = columnIndex; a.val = values; a.H = H;
    a.h_bytes = big ? 0u : (unsigned)table_bytes; a.ld_bytes = (unsigned)(ldh * es); a.big = big;
    a.D = D; a.ldd = ldd; a.plan = plan; a.stream = stream;
    a.acc_in = acc_in; a.acc_out = acc_out; a.ld_acc = ld_acc; a.fea_stage = fea_stage; a.ep = ep;
    a.partial = (float *)scratch;
    a.ldp = (int)sgx_align_up((size_t)n_feat, 4);
    if (plan && plan->n_tasks > 0) {
        if (!scratch || scratch_bytes < sgx_spmm_scratch_bytes(plan, n_feat)) return SGX_ERR_WORKSPACE;
    }
    a.vec_store = ((uintptr_t)D % 16 == 0) && ((ldd * es) % 16 == 0);
    const sgx_lane_split split = sgx_spmm_lane_split(dtype, H, ldh, n_feat, big);
    if (split.vec) {
        const int cpl = choose_cpl(plan, split.slots);
        return dtype == SGX_F16 ? launch_lpr<f16, 8>(a, split.slots, cpl) : launch_lpr<float, 4>(a, split.slots, cpl);
    }
    return dtype == SGX_F16 ? launch_lpr<f16, 1>(a, split.slots, 1) : launch_lpr<float, 1>(a, split.slots, 1);
}

extern "C" int sgx_spmm_csr(int dtype, int acc_mode, int spmm_block, int relu, int n_rows, int n_cols, int n_feat,
                            const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                            const void *H, int64_t ldh, void *D, int64_t ldd,
                            const sgx_plan *plan, void *scratch, size_t scratch_bytes, void *stream)
{
    return sgx_spmm_launch(dtype, acc_mode, spmm_block, relu, n_rows, n_cols, n_feat, rowPtr, columnIndex, values,
                           H, ldh, D, ldd, plan, scratch, scratch_bytes, (hipStream_t)stream, nullptr, nullptr, 0);
}

extern "C" int sgx_spmm_csr_acc(int dtype, int relu, int n_rows, int n_cols, int n_feat,
                                const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                const void *H, int64_t ldh, void *D, int64_t ldd,
                                const float *acc_in, float *acc_out, int64_t ld_acc,
                                const sgx_plan *plan, void *scratch, size_t scratch_bytes, void *stream)
{
    if (D && acc_out) return SGX_ERR_SHAPE;           // one destination: the final rows or the fp32 partial
    return sgx_spmm_launch(dtype, SGX_ACC_F32, 1, relu, n_rows, n_cols, n_feat, rowPtr, columnIndex, values, H, ldh, D,
                           ldd, plan, scratch, scratch_bytes, (hipStream_t)stream, acc_in, acc_out, ld_acc);
}
