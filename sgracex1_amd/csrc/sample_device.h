// What the neighbour sampler (sample.hip) and the batch preparation behind it (node_batch.hip) share: the counter block
// both read their sizes from, the three-launch exclusive scan over a functor, and the capacity bounds of a sample.
#pragma once
#include "sgx_internal.h"

namespace sgx_sample {

constexpr int kBlock = 256;
constexpr int kPer = 8;                       // items per thread of a scan workgroup (contiguous)
constexpr int kTile = kBlock * kPer;          // items per scan workgroup
constexpr int kScanTop = 1024;                // threads of the one workgroup that scans the workgroup sums
constexpr int kStatusSeeds = 1, kStatusCapacity = 2;
// the largest fan-out whose subset the sampler keeps in the wavefront's LDS slice (sample_wide_kernel, sgx_sample_form
// 2); larger ones run on one lane
constexpr int kWideMax = 1024;
// behind the sampler's counters: what the batch preparation reports through the same read-back
constexpr int kExtras = 4, kNormNnz = 0, kFeaNnz = 1, kDeadRows = 2, kMaxRow = 3;

// counter block: [0] status, then nodes(0..H), then edges(0..H), then the kExtras counts of the batch preparation
struct Counters {
    int32_t *c;
    int H;
    __device__ int32_t &status() const { return c[0]; }
    __device__ int32_t &nodes(int h) const { return c[1 + h]; }
    __device__ int32_t &edges(int h) const { return c[2 + H + h]; }
    __device__ int32_t &extra(int k) const { return c[3 + 2 * H + k]; }
    __device__ int frontier_begin(int h) const { return h ? c[h] : 0; }
};

static inline int counter_count(int n_hops) { return 2 * n_hops + 3 + kExtras; }
static inline size_t counters_bytes(int n_hops) { return sgx_align_up(sizeof(int32_t) * counter_count(n_hops), 256); }

template <int NT>
__device__ inline int block_exclusive_scan(int x, int *total)
{
    __shared__ int wsum[NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const int s = wsum[i];
        off += i < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return off + inc - x;
}

// The scan over a functor F: n() items, value(i) of each, emit(i, exclusive sum, value) and total(sum); F::ctr is the
// counter block (a set status skips everything).
template <class F>
__global__ __launch_bounds__(kBlock) void scan_reduce_kernel(F f, int32_t *__restrict__ bsum)
{
    if (f.ctr.status()) return;
    const int n = f.n(), base = blockIdx.x * kTile;
    if (base >= n) return;                                 // uniform over the workgroup
    int s = 0;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int i = base + u * kBlock + threadIdx.x;
        if (i < n) s += f.value(i);
    }
    int tot;
    block_exclusive_scan<kBlock>(s, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

template <class F>
__global__ __launch_bounds__(kScanTop) void scan_top_kernel(F f, int32_t *__restrict__ bsum)
{
    if (f.ctr.status()) return;
    const int n = f.n(), nb = (n + kTile - 1) / kTile;
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += kScanTop) {
        const int i = b0 + threadIdx.x;
        const int x = i < nb ? bsum[i] : 0;
        int tot;
        const int ex = block_exclusive_scan<kScanTop>(x, &tot);
        if (i < nb) bsum[i] = carry + ex;
        carry += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) f.total(carry);
}

template <class F>
__global__ __launch_bounds__(kBlock) void scan_emit_kernel(F f, const int32_t *__restrict__ bsum)
{
    if (f.ctr.status()) return;
    const int n = f.n(), base = blockIdx.x * kTile;
    if (base >= n) return;
    const int i0 = base + threadIdx.x * kPer;
    int v[kPer], s = 0;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        v[u] = i0 + u < n ? f.value(i0 + u) : 0;
        s += v[u];
    }
    int tot;
    int ex = block_exclusive_scan<kBlock>(s, &tot) + bsum[blockIdx.x];
#pragma unroll
    for (int u = 0; u < kPer; ++u)
        if (i0 + u < n) {
            f.emit(i0 + u, ex, v[u]);
            ex += v[u];
        }
}

// the three launches of one scan over at most `items` items
template <class F>
inline void scan_launch(const F &f, int64_t items, int32_t *bsum, hipStream_t s)
{
    int64_t g = (items + kTile - 1) / kTile;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(scan_reduce_kernel<F>, dim3((unsigned)g), dim3(kBlock), 0, s, f, bsum);
    hipLaunchKernelGGL(scan_top_kernel<F>, dim3(1), dim3(kScanTop), 0, s, f, bsum);
    hipLaunchKernelGGL(scan_emit_kernel<F>, dim3((unsigned)g), dim3(kBlock), 0, s, f, bsum);
}

// the sizes of every hop, from the fan-outs alone (sgx.h): frontier rows, sampled edges; totals
struct Bounds {
    int64_t front[64], edges[64], max_nodes, max_edges, max_tiles;
};

static inline bool bounds(int n_nodes, int64_t nnz, int B, int n_hops, const int *fanouts, Bounds *b)
{
    if (n_nodes < 0 || nnz < 0 || nnz > 0x7ffffffe || B < 0 || B > n_nodes || n_hops < 1 || n_hops > 64 || !fanouts)
        return false;
    // (a frontier is bounded by n_nodes - B, not by what the earlier bounds leave: a hop that finds fewer nodes than
    // its bound leaves more for the next one)
    int64_t front = B, nodes = B, edges = 0, tiles = 1;
    for (int h = 0; h < n_hops; ++h) {
        const int k = fanouts[h];
        if (k < -1) return false;
        int64_t e = k < 0 ? nnz : front * (int64_t)k;
        if (e > nnz) e = nnz;
        b->front[h] = front;
        b->edges[h] = e;
        const int64_t items = front > e ? front : e;
        if ((items + kTile - 1) / kTile > tiles) tiles = (items + kTile - 1) / kTile;
        edges += e;
        front = e < n_nodes - B ? e : n_nodes - B;
        nodes += front;
    }
    b->max_nodes = nodes < n_nodes ? nodes : n_nodes;
    b->max_edges = edges < nnz ? edges : nnz;
    b->max_tiles = tiles;
    return true;
}

static inline unsigned grid_of(int64_t items, int per, int64_t cap)
{
    int64_t g = (items + per - 1) / per;
    if (g < 1) g = 1;
    if (cap > 0 && g > cap) g = cap;
    return (unsigned)g;
}

// sample.hip.  sample_enqueue: every launch of sgx_sample_neighbors on its checked arguments (batch >= 1), the counter
// block `cbuf` cleared first, nothing read back.  step_dev != NULL: the sampling key is formed in the kernel from that
// device word in place of `step` (the same key for the same value), so a recorded call draws anew once the word changes.
// sample_finish: the one read-back of counter_count(n_hops) int32 and the stream synchronisation; status and hop
// counts decoded, the extras copied to `extras` (may be NULL).
int sample_enqueue(const int32_t *rowPtr, const int32_t *columnIndex, int n_nodes, const int32_t *seeds, int batch, int n_hops,
                   const int *fanouts, uint64_t seed, uint64_t step, const uint64_t *step_dev, int32_t *node_map, int32_t *n_id,
                   int32_t *out_rowPtr, int32_t *out_col, int32_t *edge_pos, int64_t max_nodes, int64_t max_edges, const Bounds &b,
                   int32_t *cbuf, int32_t *bsum, hipStream_t s);
int sample_finish(const int32_t *cbuf, int n_hops, int64_t *hop_nodes, int64_t *hop_edges, int32_t *extras, hipStream_t s);

}  // namespace sgx_sample
