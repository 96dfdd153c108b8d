// sgx_csr_transpose: the CSR of A^T, stable (rule in include/sgx.h).
//
// A least-significant-digit radix sort of the stored entries' positions keyed by column index, 8 bits a pass:
// ceil(bits(n_cols - 1) / 8) passes (at least one).  A pass is three launches over tiles of kTile entries:
//   hist    : the tile's count per digit, counts[digit][tile]
//   scan    : workgroup d scans row d of counts over the tiles in place (exclusive) and leaves the digit's total
//   scatter : every entry to  base[digit] + counts[digit][tile] + its rank among the tile's entries of that digit,
//             base = the exclusive scan of the 256 totals (each workgroup forms it again: 256 values)
// The rank keeps the pass stable: a wavefront owns kRounds * 64 consecutive entries and takes them 64 at a time; inside
// a round a lane's rank among equal digits is the population count of the lower lanes with the same digit (eight ballots
// give that mask), the rounds before it and the wavefronts before it add their counts through LDS.  Nothing depends on
// the order in which an atomic returns: the histogram only counts.  The last pass stores the outputs themselves -- order,
// values_t, columnIndex_t (the source row: a binary search of rowPtr per entry) -- and the sorted keys, from which one more
// launch takes rowPtr_t[c] = the first sorted position whose key is not below c.  Work: O(nnz * passes + n_cols log nnz),
// whatever the lengths of the rows of A^T.
#include "sgx_internal.h"

namespace {

constexpr int kTile = SGX_CSR_TRANSPOSE_TILE;
constexpr int kBlock = 256, kWaves = kBlock / 64, kRadix = 256;
constexpr int kRounds = kTile / kBlock;             // rounds of 64 entries per wavefront
static_assert(kTile % kBlock == 0 && kRadix == kBlock, "a thread per digit, whole rounds per wavefront");

// the lanes of this wavefront that hold a valid entry with the same digit (meaningful on valid lanes)
__device__ __forceinline__ unsigned long long digit_peers(int d, bool valid)
{
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot((d >> b) & 1);
        peers &= ((d >> b) & 1) ? m : ~m;
    }
    return peers;
}

// exclusive scan of one value per thread over the workgroup; total = the sum of all
__device__ __forceinline__ int block_exclusive_scan(int v, int *wave_sums, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                 // (wave_sums may still be read by a scan before this one)
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int s = wave_sums[w];
        base += w < wave ? s : 0;
        total += s;
    }
    return base + inc - v;
}

__device__ __forceinline__ int digit_of(int32_t key, int shift) { return (int)(((uint32_t)key >> shift) & (kRadix - 1)); }

__global__ __launch_bounds__(kBlock) void csr_transpose_hist_kernel(const int32_t *keys, int64_t nnz, int shift, int tiles,
                                                                     int32_t *counts)
{
    __shared__ int h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kTile;
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = base + r * kBlock + threadIdx.x;
        const bool valid = i < nnz;
        const int d = valid ? digit_of(keys[i], shift) : 0;
        const unsigned long long peers = digit_peers(d, valid);
        // one add per digit, wavefront and round: a column that holds the whole tile does not serialise 2048 adds
        if (valid && (peers & ((1ull << lane) - 1)) == 0) atomicAdd(&h[d], __popcll(peers));
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void csr_transpose_scan_kernel(int32_t *counts, int tiles, int32_t *totals)
{
    __shared__ int wave_sums[kWaves];
    int32_t *row = counts + (size_t)blockIdx.x * tiles;
    int carry = 0;
    for (int t0 = 0; t0 < tiles; t0 += kBlock) {
        const int t = t0 + threadIdx.x;
        const int v = t < tiles ? row[t] : 0;
        int total;
        const int ex = block_exclusive_scan(v, wave_sums, total);
        if (t < tiles) row[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// the row of A that holds stored entry p: the last r with rowPtr[r] <= p (n_rows >= 1)
__device__ __forceinline__ int row_of(const int32_t *rowPtr, int n_rows, int p)
{
    int lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (rowPtr[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct scatter_args {
    const int32_t *keys_in, *pos_in;     // FIRST: keys_in = columnIndex, the positions are 0 .. nnz-1
    int32_t *keys_out, *pos_out;         // LAST: pos_out = order (may be NULL)
    const int32_t *counts, *totals;
    int64_t nnz;
    int shift, tiles;
    // LAST only
    const int32_t *rowPtr;
    int n_rows, value_bytes;             // 0: a pattern
    const void *values;
    void *values_t;
    int32_t *columnIndex_t;
};

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kBlock) void csr_transpose_scatter_kernel(scatter_args a)
{
    __shared__ int cnt[kWaves][kRadix];
    __shared__ int wave_sums[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();

    volatile int *mine = cnt[wave];      // (volatile: lanes of one wavefront hand counts to each other from round to round)
    const int64_t wbase = (int64_t)blockIdx.x * kTile + (int64_t)wave * (kRounds * 64);
    int32_t key[kRounds], pos[kRounds];
    int rank[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = wbase + r * 64 + lane;
        const bool valid = i < a.nnz;
        key[r] = valid ? a.keys_in[i] : 0;
        pos[r] = FIRST ? (int32_t)i : (valid ? a.pos_in[i] : 0);
        const int d = digit_of(key[r], a.shift);
        const unsigned long long peers = digit_peers(d, valid);
        const unsigned long long below = peers & ((1ull << lane) - 1);
        const int c = valid ? mine[d] : 0;           // what the rounds before this one counted
        rank[r] = c + __popcll(below);
        if (valid && below == 0) mine[d] = c + __popcll(peers);
    }
    __syncthreads();

    // thread d: where digit d of this tile begins, then where each wavefront's share of it begins
    int all;
    int o = block_exclusive_scan(a.totals[threadIdx.x], wave_sums, all) + a.counts[(size_t)threadIdx.x * a.tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int c = cnt[w][threadIdx.x];
        cnt[w][threadIdx.x] = o;
        o += c;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = wbase + r * 64 + lane;
        if (i >= a.nnz) continue;
        const int dest = mine[digit_of(key[r], a.shift)] + rank[r];
        a.keys_out[dest] = key[r];
        if (!LAST) {
            a.pos_out[dest] = pos[r];
        } else {
            if (a.pos_out) a.pos_out[dest] = pos[r];
            a.columnIndex_t[dest] = row_of(a.rowPtr, a.n_rows, pos[r]);
            if (a.value_bytes == 2) ((uint16_t *)a.values_t)[dest] = ((const uint16_t *)a.values)[pos[r]];
            else if (a.value_bytes == 4) ((uint32_t *)a.values_t)[dest] = ((const uint32_t *)a.values)[pos[r]];
        }
    }
}

__global__ __launch_bounds__(kBlock) void csr_transpose_rowptr_kernel(const int32_t *sorted, int64_t nnz, int n_cols,
                                                                       int32_t *rowPtr_t)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c > n_cols) return;
    int64_t lo = 0, hi = nnz;                        // the first sorted position whose key is not below c
    if (c == n_cols) lo = nnz;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    rowPtr_t[c] = (int32_t)lo;
}

struct transpose_layout {
    size_t keys[2], pos[2], counts, totals, total;
    int tiles;
};

bool layout_of(int n_rows, int n_cols, int64_t nnz, transpose_layout &l)
{
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || nnz > INT32_MAX) return false;
    const size_t per = sgx_align_up((size_t)(nnz > 0 ? nnz : 1) * sizeof(int32_t), 256);
    l.tiles = (int)((nnz + kTile - 1) / kTile);
    l.keys[0] = 0;
    l.keys[1] = per;
    l.pos[0] = 2 * per;
    l.pos[1] = 3 * per;
    l.counts = 4 * per;
    l.totals = l.counts + sgx_align_up((size_t)(l.tiles > 0 ? l.tiles : 1) * kRadix * sizeof(int32_t), 256);
    l.total = l.totals + sgx_align_up(kRadix * sizeof(int32_t), 256);
    return true;
}

}   // namespace

extern "C" size_t sgx_csr_transpose_workspace_bytes(int n_rows, int n_cols, int64_t nnz)
{
    transpose_layout l;
    return layout_of(n_rows, n_cols, nnz, l) ? l.total : 0;
}

extern "C" int sgx_csr_transpose(int dtype_values, int n_rows, int n_cols, int64_t nnz, const int32_t *rowPtr,
                                 const int32_t *columnIndex, const void *values, int32_t *rowPtr_t, int32_t *columnIndex_t,
                                 void *values_t, int32_t *order, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rowPtr || !columnIndex || !rowPtr_t || !columnIndex_t || (values == nullptr) != (values_t == nullptr)) return SGX_ERR_NULL;
    if (n_rows < 0 || n_cols < 0 || nnz < 0) return SGX_ERR_SHAPE;
    if (nnz > INT32_MAX || (values && dtype_values != SGX_F16 && dtype_values != SGX_F32)) return SGX_ERR_UNSUPPORTED;
    transpose_layout l;
    layout_of(n_rows, n_cols, nnz, l);
    if (!workspace || workspace_bytes < l.total) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256 != 0) return SGX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int32_t *keys[2] = {(int32_t *)(ws + l.keys[0]), (int32_t *)(ws + l.keys[1])};
    int32_t *pos[2] = {(int32_t *)(ws + l.pos[0]), (int32_t *)(ws + l.pos[1])};
    int32_t *counts = (int32_t *)(ws + l.counts), *totals = (int32_t *)(ws + l.totals);
    const unsigned rowptr_grid = (unsigned)(((int64_t)n_cols + 1 + kBlock - 1) / kBlock);
    if (n_rows == 0 || nnz == 0) {                   // nothing stored: rowPtr_t all zeros
        hipLaunchKernelGGL(csr_transpose_rowptr_kernel, dim3(rowptr_grid), dim3(kBlock), 0, s, keys[0], (int64_t)0, n_cols, rowPtr_t);
        SGX_LAUNCH_CHECK();
        return SGX_OK;
    }

    int bits = 0;
    while (bits < 31 && ((int64_t)1 << bits) < (int64_t)n_cols) ++bits;      // bits(n_cols - 1)
    const int passes = bits <= 8 ? 1 : (bits + 7) / 8;
    scatter_args a;
    a.counts = counts, a.totals = totals, a.nnz = nnz, a.tiles = l.tiles;
    a.rowPtr = rowPtr, a.n_rows = n_rows, a.value_bytes = values ? (int)sgx_elem_size(dtype_values) : 0;
    a.values = values, a.values_t = values_t, a.columnIndex_t = columnIndex_t;
    for (int p = 0; p < passes; ++p) {
        const bool first = p == 0, last = p == passes - 1;
        a.shift = 8 * p;
        a.keys_in = first ? columnIndex : keys[(p + 1) & 1];
        a.pos_in = first ? nullptr : pos[(p + 1) & 1];
        a.keys_out = keys[p & 1];
        a.pos_out = last ? order : pos[p & 1];
        hipLaunchKernelGGL(csr_transpose_hist_kernel, dim3(l.tiles), dim3(kBlock), 0, s, a.keys_in, nnz, a.shift, l.tiles, counts);
        SGX_LAUNCH_CHECK();
        hipLaunchKernelGGL(csr_transpose_scan_kernel, dim3(kRadix), dim3(kBlock), 0, s, counts, l.tiles, totals);
        SGX_LAUNCH_CHECK();
        if (first && last) hipLaunchKernelGGL((csr_transpose_scatter_kernel<true, true>), dim3(l.tiles), dim3(kBlock), 0, s, a);
        else if (first) hipLaunchKernelGGL((csr_transpose_scatter_kernel<true, false>), dim3(l.tiles), dim3(kBlock), 0, s, a);
        else if (last) hipLaunchKernelGGL((csr_transpose_scatter_kernel<false, true>), dim3(l.tiles), dim3(kBlock), 0, s, a);
        else hipLaunchKernelGGL((csr_transpose_scatter_kernel<false, false>), dim3(l.tiles), dim3(kBlock), 0, s, a);
        SGX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(csr_transpose_rowptr_kernel, dim3(rowptr_grid), dim3(kBlock), 0, s, keys[(passes - 1) & 1], nnz, n_cols, rowPtr_t);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
