// The attention gradient of the GAT backward by stored entries (sgx_gat_attention_grad_flat, sgx.h): the outputs of
// sgx_gat_attention_grad (layer_bwd.hip) on a schedule that depends on the entry capacity, the row count, F and Wh's
// alignment alone.  Neither half has rows:
//     grad_attention[0:F]  = sum_r g1[r] Wh[r]                 a reduction over the rows
//     grad_attention[F:2F] = sum_{e < end} sg_e Wh[col_e]      a reduction over the stored entries
// so both are cut into units of T = kFlatChunk consecutive items (flat_device.h), a wavefront per unit, and no search in
// rowPtr is needed: the entry chunks [0, ceil(nnz / T)) first, then the row chunks.  A hub row is spread over the chunks
// its entries fall in like any other run of entries -- the walk sgx_gat_attention_grad leaves to one workgroup.
//   * end = min(rowPtr[n_rows], nnz) is read on the device; an entry chunk at or behind it leaves at once and writes
//     nothing, and the second launch bounds itself by the same end: what lies behind it is never read.
//   * inside a unit LPR lanes (16 bytes of a Wh row each) form a lane group, 64 / LPR groups to the wavefront; group g
//     takes items g, g + 64 / LPR, ... of the unit in ascending order, one fp32 fma per item and column onto +0, with K
//     gathers in flight; the groups' sums are added in group order (lane shuffles: the wavefronts share nothing) and the
//     unit's partial row [F] goes to the workspace by plain 16-byte stores.
//   * the second launch, 16 columns to a workgroup: thread (q, j) adds column j of the units q, q + 16, ... in ascending
//     order from +0, four loads in flight; the 16 chains are added in order q through LDS and the element is stored once.
// No atomics, no LDS in the first launch, nothing allocated, no synchronisation: capturable; the same bits on every run and
// at every capacity nnz >= rowPtr[n_rows].
#include "sgx_device.h"
#include "flat_device.h"          // T and the chunk count

namespace {

constexpr int kFinCols = 16;                        // columns a workgroup of the second launch adds ...
constexpr int kFinChains = kBlock / kFinCols;       // ... in this many interleaved chains over the units

static inline int64_t agf_row_chunks(int n_rows) { return ((int64_t)n_rows + kFlatChunk - 1) / kFlatChunk; }

// Four columns of a Wh row at byte offset `at`: 16 bytes (VEC), or the first n_left (<= 4) of them one element at a time;
// kOOB, the elements not asked for and whatever lies past the table read 0
template <bool VEC>
__device__ __forceinline__ void agf_load4(__amdgpu_buffer_rsrc_t rsrc, unsigned at, int n_left, float *w)
{
    union { u32x4 v; float f[4]; } u;
    if constexpr (VEC) {
        u.v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, at, 0, 0);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) u.v[i] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (at == kOOB || i >= n_left) ? kOOB : at + 4u * i, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = u.f[i];
}

// t[0..3] += sum over the unit's items k = k0, k0 + step, ... < count of s[k] Wh[idx_k][col0 .. col0 + 3], one fma per item
// and column in that order, K gathers in flight.  idx_k = first_row + k for a row chunk (col == nullptr), col[k] otherwise;
// s and col point at the unit's first item.
template <bool VEC, int K>
__device__ __forceinline__ void agf_chain(__amdgpu_buffer_rsrc_t w_rsrc, const int32_t *__restrict__ col, const float *__restrict__ s,
                                          int first_row, int k0, int step, int count, unsigned ldw_bytes, unsigned col_bytes, int n_left,
                                          float *t)
{
    for (int k = k0; k < count; k += K * step) {
        float sv[K], w[K][4];
#pragma unroll
        for (int j = 0; j < K; ++j) {                           // K rows in flight, added in order below
            const int kj = k + j * step;
            const bool have = kj < count;
            const int idx = col == nullptr ? first_row + kj : (have ? col[kj] : 0);
            sv[j] = have ? s[kj] : 0.0f;
            agf_load4<VEC>(w_rsrc, (have && col_bytes != kOOB) ? (unsigned)idx * ldw_bytes + col_bytes : kOOB, n_left, w[j]);
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (k + j * step < count) {
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = __builtin_fmaf(sv[j], w[j][i], t[i]);
            }
    }
}

// partial: [n_echunks + row chunks][ldp] fp32, the entry chunks first
template <int LPR, bool VEC>
__global__ __launch_bounds__(kBlock) void attention_grad_flat_kernel(
    int n_rows, int n_feat, int nnz_cap, int n_echunks, int n_units, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ sg, const float *__restrict__ g1, const float *__restrict__ Wh, unsigned w_bytes, unsigned ldw_bytes,
    float *__restrict__ partial, int ldp)
{
    constexpr int GROUPS = 64 / LPR;               // lane groups of the wavefront
    constexpr int TILE = LPR * 4;                  // columns a lane group covers per pass
    constexpr int K = kFlatChunk / GROUPS < 8 ? kFlatChunk / GROUPS : 8;      // gathers in flight: a group's whole share at LPR = 1
    constexpr int kGroupUnroll = GROUPS <= 8 ? GROUPS : 1;                    // (63 unrolled steps of shuffles cost 100 registers)
    const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
    if (u >= n_units) return;
    const int lane = threadIdx.x & 63, sub = lane % LPR, grp = lane / LPR;

    const int32_t *u_col = nullptr;
    const float *u_s;
    int first_row = 0, count;
    if (u < n_echunks) {
        // the matrix's own end, read here: nnz_cap is a bound on it (and what the arrays hold, so never read past it)
        int end = n_rows > 0 ? rowptr[n_rows] : 0;
        end = end < 0 ? 0 : (end > nnz_cap ? nnz_cap : end);
        const int64_t lo = (int64_t)u * kFlatChunk;
        if (lo >= end) return;                                     // a chunk of the capacity behind the end
        count = end - lo < kFlatChunk ? (int)(end - lo) : kFlatChunk;
        u_col = col + lo;
        u_s = sg + lo;
    } else {
        const int64_t lo = (int64_t)(u - n_echunks) * kFlatChunk;
        count = n_rows - lo < kFlatChunk ? (int)(n_rows - lo) : kFlatChunk;
        first_row = (int)lo;
        u_s = g1 + lo;
    }

    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wh), 0, w_bytes, 0x00020000);
    float *__restrict__ row = partial + (size_t)u * (size_t)ldp;
    for (int c0 = 0; c0 < n_feat; c0 += TILE) {
        const int col0 = c0 + sub * 4;
        const bool col_in = col0 < n_feat;
        float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        agf_chain<VEC, K>(w_rsrc, u_col, u_s, first_row, grp, GROUPS, count, ldw_bytes, col_in ? (unsigned)col0 * 4u : kOOB, n_feat - col0, t);
        // the groups' sums in group order; every lane follows the columns of its place in the group
        float4 tot = make_float4(t[0], t[1], t[2], t[3]);
        if constexpr (GROUPS > 1) {
            tot.x = __shfl(t[0], sub); tot.y = __shfl(t[1], sub); tot.z = __shfl(t[2], sub); tot.w = __shfl(t[3], sub);
#pragma unroll kGroupUnroll
            for (int g = 1; g < GROUPS; ++g) {
                tot.x += __shfl(t[0], g * LPR + sub); tot.y += __shfl(t[1], g * LPR + sub);
                tot.z += __shfl(t[2], g * LPR + sub); tot.w += __shfl(t[3], g * LPR + sub);
            }
        }
        if (grp == 0 && col_in) *reinterpret_cast<float4 *>(row + col0) = tot;     // (ldp is a multiple of 4: col0 + 3 < ldp)
    }
}

// out[half F + j] = the live units' partials of column j: 16 chains by unit index, then the chains in order
__global__ __launch_bounds__(kBlock) void attention_grad_flat_finish_kernel(
    int n_rows, int n_feat, int nnz_cap, int n_echunks, int n_rchunks, const int32_t *__restrict__ rowptr, const float *__restrict__ partial,
    int ldp, float *__restrict__ out)
{
    __shared__ float part[kFinChains][kFinCols];
    const int blocks_per_half = (n_feat + kFinCols - 1) / kFinCols;
    const int half = (int)blockIdx.x / blocks_per_half;             // 0: the rows' half, 1: the entries'
    const int jj = threadIdx.x % kFinCols, q = threadIdx.x / kFinCols;
    const int j = ((int)blockIdx.x % blocks_per_half) * kFinCols + jj;
    int n_live = n_rchunks;
    const float *__restrict__ base = partial + (size_t)n_echunks * (size_t)ldp;
    if (half == 1) {
        int end = n_rows > 0 ? rowptr[n_rows] : 0;
        end = end < 0 ? 0 : (end > nnz_cap ? nnz_cap : end);
        n_live = (int)(((int64_t)end + kFlatChunk - 1) / kFlatChunk);          // the chunks the first launch wrote
        n_live = n_live > n_echunks ? n_echunks : n_live;
        base = partial;
    }
    float t = 0.0f;
    if (j < n_feat)
        for (int c = q; c < n_live; c += 4 * kFinChains) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {                            // four units in flight, added in order below
                const int ci = c + i * kFinChains;
                v[i] = ci < n_live ? base[(size_t)ci * (size_t)ldp + j] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c + i * kFinChains < n_live) t += v[i];
        }
    part[q][jj] = t;
    __syncthreads();
    if (q == 0 && j < n_feat) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < kFinChains; ++k) s += part[k][jj];
        out[(size_t)half * n_feat + j] = s;
    }
}

struct AgfArgs {
    int n_rows, n_feat, nnz, n_echunks, n_units;
    const int32_t *rowptr, *col;
    const float *sg, *g1, *Wh;
    unsigned w_bytes, ldw_bytes;
    float *partial;
    int ldp;
    hipStream_t stream;
};

template <int LPR, bool VEC>
int agf_launch(const AgfArgs &a)
{
    constexpr int kWaves = kBlock / 64;
    hipLaunchKernelGGL((attention_grad_flat_kernel<LPR, VEC>), dim3((unsigned)((a.n_units + kWaves - 1) / kWaves)), dim3(kBlock), 0, a.stream,
                       a.n_rows, a.n_feat, a.nnz, a.n_echunks, a.n_units, a.rowptr, a.col, a.sg, a.g1, a.Wh, a.w_bytes, a.ldw_bytes,
                       a.partial, a.ldp);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

template <int LPR>
int agf_launch_vec(const AgfArgs &a, bool vec) { return vec ? agf_launch<LPR, true>(a) : agf_launch<LPR, false>(a); }

}  // namespace

extern "C" size_t sgx_gat_attention_grad_flat_workspace_bytes(int64_t nnz, int n_rows, int n_feat)
{
    if (nnz < 0 || nnz > kFlatMaxNnz || n_rows < 0 || n_feat < 1) return 0;
    return sgx_align_up((size_t)(flat_chunks(nnz) + agf_row_chunks(n_rows)) * (size_t)flat_ldp(n_feat) * sizeof(float), 256);
}

extern "C" int sgx_gat_attention_grad_flat(int n_rows, int n_cols, int n_feat, int64_t nnz, const int32_t *rowPtr,
                                           const int32_t *columnIndex, const float *sg, const float *g1, const float *Wh, int64_t ldw,
                                           float *grad_attention, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_rows < 0 || n_cols < n_rows || n_feat < 1 || ldw < n_feat || nnz < 0 || nnz > kFlatMaxNnz) return SGX_ERR_SHAPE;
    if (!grad_attention) return SGX_ERR_NULL;
    if (n_rows > 0 && (!rowPtr || !columnIndex || !sg || !g1 || !Wh)) return SGX_ERR_NULL;
    const unsigned long long w_bytes = (unsigned long long)n_cols * (unsigned long long)ldw * 4ull;
    if (w_bytes >= 0xFFFFFFF0ull) return SGX_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < sgx_gat_attention_grad_flat_workspace_bytes(nnz, n_rows, n_feat)) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256 != 0) return SGX_ERR_ALIGN;

    AgfArgs a;
    a.n_rows = n_rows; a.n_feat = n_feat; a.nnz = (int)nnz;
    a.n_echunks = (int)flat_chunks(nnz);
    const int n_rchunks = (int)agf_row_chunks(n_rows);
    a.n_units = a.n_echunks + n_rchunks;
    a.rowptr = rowPtr; a.col = columnIndex; a.sg = sg; a.g1 = g1; a.Wh = Wh;
    a.w_bytes = (unsigned)w_bytes; a.ldw_bytes = (unsigned)(ldw * 4);
    a.partial = (float *)workspace; a.ldp = flat_ldp(n_feat); a.stream = (hipStream_t)stream;
    const bool vec = (uintptr_t)Wh % 16 == 0 && (ldw * 4) % 16 == 0;
    int lpr = sgx_next_pow2((n_feat + 3) / 4);
    if (lpr > 64) lpr = 64;
    int rc;
    switch (lpr) {
    case 1: rc = agf_launch_vec<1>(a, vec); break;
    case 2: rc = agf_launch_vec<2>(a, vec); break;
    case 4: rc = agf_launch_vec<4>(a, vec); break;
    case 8: rc = agf_launch_vec<8>(a, vec); break;
    case 16: rc = agf_launch_vec<16>(a, vec); break;
    case 32: rc = agf_launch_vec<32>(a, vec); break;
    default: rc = agf_launch_vec<64>(a, vec); break;
    }
    if (rc != SGX_OK) return rc;
    const unsigned fin_blocks = 2u * (unsigned)((n_feat + kFinCols - 1) / kFinCols);
    hipLaunchKernelGGL(attention_grad_flat_finish_kernel, dim3(fin_blocks), dim3(kBlock), 0, a.stream, n_rows, n_feat, a.nnz, a.n_echunks,
                       n_rchunks, rowPtr, (const float *)a.partial, a.ldp, grad_attention);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
