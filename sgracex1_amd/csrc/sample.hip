// Neighbour sampling for mini-batch training: the NeighborLoader call pattern of the reference's demo
// (demo/emulation/demo_sgrace.py:112-125, `full_graph = 0`).  The rule -- Floyd's k-subset per frontier row, the
// counter-based draw, the relabel order -- is written down in include/sgx.h; this file is its device form.
//
// One hop is eight launches, each reading the sizes it needs from the counter block in the workspace (so nothing is
// read back between hops; every grid is sized on the host from the bound):
//   1-3  row counts of the frontier -> exclusive scan -> out_rowPtr of the frontier rows     (scan_*<RowCounts>)
//   4    one wavefront per frontier row: Floyd's subset, positions in ascending order, global column ids,
//        atomicMin of each slot's ordinal into node_map[column]                              (sample_kernel; for a
//        fan-out of 65 .. kWideMax sample_wide_kernel, the same rule with the subset in LDS: sgx_sample_form)
//   5-7  first-appearance flags (node_map[column] == own slot) -> exclusive scan -> new local ids; the first slot of a
//        node writes n_id and stores -(id + 1) in node_map                                   (scan_*<FirstSeen>)
//   8    columns relabelled through node_map                                                 (relabel_kernel)
// Kernel boundaries are the only ordering between workgroups.  A tail writes the row pointer of the last hop's new
// nodes, and the map entries of every node of n_id are put back to the sentinel.
// The counter block, the scan and the capacity bounds are in sample_device.h, shared with node_batch.hip.
#include "sample_device.h"
#include "tail_device.h"

using namespace sgx_sample;

namespace {

constexpr int kFast = 64;                     // fan-outs up to this keep the subset in registers, one element per lane
constexpr int32_t kSentinel = 0x7fffffff;

using sgx_tail::mix64;                        // the splitmix64 finaliser, which the tail's dropout hashes with too

__device__ inline int draw(uint64_t key, int v, int j)
{
    const uint64_t w = ((uint64_t)(uint32_t)v << 32) | (uint32_t)j;
    return (int)__umul64hi(mix64(key ^ mix64(w)), (uint64_t)j + 1);     // in [0, j]
}

// items: the frontier rows of hop h; value: the number of edges the row samples
struct RowCounts {
    Counters ctr;
    const int32_t *rowPtr, *n_id;
    int32_t *out_rowPtr;
    int h, k;
    __device__ int n() const { return ctr.nodes(h) - ctr.frontier_begin(h); }
    __device__ int value(int i) const
    {
        const int v = n_id[ctr.frontier_begin(h) + i];
        const int deg = rowPtr[v + 1] - rowPtr[v];
        return (k < 0 || deg <= k) ? deg : k;
    }
    __device__ void emit(int i, int excl, int) const { out_rowPtr[ctr.frontier_begin(h) + i] = ctr.edges(h) + excl; }
    __device__ void total(int t) const { ctr.edges(h + 1) = ctr.edges(h) + t; }
};

// items: the slots sampled at hop h; value: 1 where the slot is the first appearance of its node in this hop
struct FirstSeen {
    Counters ctr;
    const int32_t *col;
    int32_t *map, *n_id;
    int64_t max_nodes;
    int h;
    __device__ int n() const { return ctr.edges(h + 1) - ctr.edges(h); }
    __device__ int value(int i) const
    {
        const int s = ctr.edges(h) + i;
        return map[col[s]] == s;
    }
    __device__ void emit(int i, int excl, int flag) const
    {
        if (!flag) return;
        const int id = ctr.nodes(h) + excl;
        const int c = col[ctr.edges(h) + i];
        if (id >= max_nodes) {
            atomicOr(&ctr.status(), kStatusCapacity);
            return;
        }
        n_id[id] = c;
        map[c] = -(id + 1);
    }
    __device__ void total(int t) const { ctr.nodes(h + 1) = ctr.nodes(h) + t; }
};

__global__ __launch_bounds__(kBlock) void clear_kernel(int32_t *__restrict__ c, int n)
{
    for (int i = threadIdx.x; i < n; i += kBlock) c[i] = 0;
}

__global__ __launch_bounds__(kBlock) void seed_kernel(const int32_t *__restrict__ seeds, int B, int n_nodes,
                                                      int32_t *__restrict__ map, int32_t *__restrict__ n_id, Counters ctr)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) ctr.nodes(0) = B;
    if (i >= B) return;
    const int v = seeds[i];
    n_id[i] = v;
    if (v < 0 || v >= n_nodes || atomicCAS(&map[v], kSentinel, -(i + 1)) != kSentinel)
        atomicOr(&ctr.status(), kStatusSeeds);
}

struct SampleArgs {
    const int32_t *rowPtr, *colIdx, *n_id, *out_rowPtr;
    int32_t *out_col, *edge_pos, *map;
    int64_t max_edges;
    uint64_t key;                             // of (seed, step, h), formed on the host; or, with step_dev:
    const uint64_t *step_dev;                 // the step word on the device, and seed_mix = mix64(seed)
    uint64_t seed_mix;
    int h, k;
    __device__ uint64_t hop_key() const { return step_dev ? mix64(mix64(seed_mix ^ *step_dev) ^ (uint64_t)h) : key; }
};

__device__ inline void put(const SampleArgs &a, int slot, int pos)
{
    const int c = a.colIdx[pos];
    a.edge_pos[slot] = pos;
    a.out_col[slot] = c;
    atomicMin(&a.map[c], slot);
}

// one wavefront per frontier row
__global__ __launch_bounds__(kBlock) void sample_kernel(SampleArgs a, Counters ctr)
{
    if (ctr.status()) return;
    const int f0 = ctr.frontier_begin(a.h);
    const int r = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r >= ctr.nodes(a.h) - f0) return;                  // uniform over the wavefront
    const int lane = threadIdx.x & 63;
    const int v = a.n_id[f0 + r];
    const int p0 = a.rowPtr[v], deg = a.rowPtr[v + 1] - p0;
    const int off = a.out_rowPtr[f0 + r];
    const int k = a.k;
    const uint64_t key = a.hop_key();                      // uniform over the grid
    const bool all = k < 0 || deg <= k;
    if ((int64_t)off + (all ? deg : k) > a.max_edges) {
        if (lane == 0) atomicOr(&ctr.status(), kStatusCapacity);
        return;
    }
    if (all) {
        for (int p = lane; p < deg; p += 64) put(a, off + p, p0 + p);
    } else if (k <= kFast) {
        // Floyd: lane i draws for j = deg - k + i; the insertions run in order, membership by ballot
        const int j = deg - k + lane;
        const int t = lane < k ? draw(key, v, j) : -1;
        int elem = -1;
        for (int i = 0; i < k; ++i) {
            const int ti = __shfl(t, i, 64);
            const bool hit = __ballot(lane < i && elem == ti) != 0;
            if (lane == i) elem = hit ? j : ti;
        }
        int rank = 0;                                      // ascending order: rank among the k distinct positions
        for (int l = 0; l < k; ++l) rank += __shfl(elem, l, 64) < elem;
        if (lane < k) put(a, off + rank, p0 + elem);
    } else if (lane == 0) {
        // fan-outs over 64: the same rule on one lane, the subset kept in the row's own edge_pos slots (O(k^2))
        int32_t *set = a.edge_pos + off;
        for (int i = 0; i < k; ++i) {
            const int j = deg - k + i, t = draw(key, v, j);
            bool hit = false;
            for (int l = 0; l < i; ++l) hit |= set[l] == t;
            set[i] = hit ? j : t;
        }
        for (int i = 1; i < k; ++i) {
            const int x = set[i];
            int l = i - 1;
            for (; l >= 0 && set[l] > x; --l) set[l + 1] = set[l];
            set[l + 1] = x;
        }
        for (int i = 0; i < k; ++i) put(a, off + i, p0 + set[i]);
    }
}

// the lanes of a wavefront hand values to one another through its own LDS slice: LDS operations of one wavefront
// complete in order, the fences keep the compiler from moving them across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int32_t kHitBit = (int32_t)0x80000000;

// The wide form: fan-outs kFast < k <= kWideMax (sgx_sample_form 2), one wavefront per frontier row as sample_kernel,
// element i = 64 c + lane of chunk c < C = ceil(k / 64).  Floyd's loop restated so that no element waits for the one
// before it (tests/_sampler_wide_ref.py is the same in numpy), with base = deg - k, j_i = base + i, t_i = draw(j_i):
//   dup_i  = t_i is among t_0 .. t_{i-1}
//   par_i  = t_i - base where 0 <= t_i - base < i, else none   (j_par is the only j that t_i can equal)
//   hit_i  = dup_i or hit[par_i]                               = Floyd's "t_i is in S": an earlier element is t_i either
//                                                                as its own draw (dup) or as its j, which it took on a hit
//   elem_i = hit_i ? j_i : t_i
// par_i < i, so hit is the OR of dup along a chain of falling indices: ceil(log2 k) rounds of pointer jumping over the
// word (hit << 31 | par + 1), updated in place chunk by chunk -- a word read is whole, either version of it covers
// its chain up to the parent it names, and the covered length at least doubles per round.  Then the rank of every
// element among all of them gives its slot.
// LDS: two int32 [kWideMax] arrays per wavefront (the draws, later the elements; the chain words) = 8 KiB, 32 KiB static
// per workgroup of four rows: five workgroups = 20 wavefronts per CU, 5 per SIMD.  The slices are wavefront-private and
// ordered by wave_lds_sync alone: the kernel has no workgroup barrier, so the early returns are free.  Every trip
// count is a function of k (and the chunk index) alone; nothing of the subset touches global memory.
__global__ __launch_bounds__(kBlock) void sample_wide_kernel(SampleArgs a, Counters ctr)
{
    __shared__ __attribute__((aligned(16))) int32_t s_val[kBlock / 64][kWideMax];
    __shared__ __attribute__((aligned(16))) int32_t s_link[kBlock / 64][kWideMax];
    if (ctr.status()) return;
    const int f0 = ctr.frontier_begin(a.h);
    const int r = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r >= ctr.nodes(a.h) - f0) return;                  // uniform over the wavefront
    const int lane = threadIdx.x & 63;
    const int v = a.n_id[f0 + r];
    const int p0 = a.rowPtr[v], deg = a.rowPtr[v + 1] - p0;
    const int off = a.out_rowPtr[f0 + r];
    const int k = a.k;                                     // kFast < k <= kWideMax: sample_enqueue launches nothing else here
    const uint64_t key = a.hop_key();
    const bool all = deg <= k;
    if ((int64_t)off + (all ? deg : k) > a.max_edges) {
        if (lane == 0) atomicOr(&ctr.status(), kStatusCapacity);
        return;
    }
    if (all) {
        for (int p = lane; p < deg; p += 64) put(a, off + p, p0 + p);
        return;
    }
    int32_t *val = s_val[threadIdx.x >> 6], *link = s_link[threadIdx.x >> 6];
    const int4 *val4 = (const int4 *)val;
    const int C = (k + 63) >> 6, base = deg - k;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {                          // slots k .. 64 C - 1 hold -1, which no draw equals
        const int i = c * 64 + lane;
        val[i] = i < k ? draw(key, v, base + i) : -1;
    }
    wave_lds_sync();
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const int i = c * 64 + lane, t = val[i];
        unsigned diff = 1;                                 // the chunks before this one, every index below i: 0 once a draw equals t
#pragma unroll 2
        for (int g = 0; g < c * 16; ++g) {
            const int4 x = val4[g];
            diff = min(min(diff, (unsigned)(x.x ^ t)), min((unsigned)(x.y ^ t), min((unsigned)(x.z ^ t), (unsigned)(x.w ^ t))));
        }
        int first = i;                                     // this chunk: the first index that holds t, i itself at the latest
#pragma unroll 2
        for (int g = c * 16; g < c * 16 + 16; ++g) {
            const int4 x = val4[g];
            const int l = 4 * g;
            first = min(min(first, x.x == t ? l : i), min(x.y == t ? l + 1 : i, min(x.z == t ? l + 2 : i, x.w == t ? l + 3 : i)));
        }
        const bool dup = diff == 0 || first < i;
        const int par = t - base;
        link[i] = (dup ? kHitBit : 0) | (par >= 0 && par < i ? par + 1 : 0);
    }
    wave_lds_sync();
    const int rounds = 32 - __clz(k - 1);                  // ceil(log2 k)
#pragma unroll 1
    for (int round = 0; round < rounds; ++round) {
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            const int i = c * 64 + lane;
            const int32_t w = link[i];
            const int par = (w & ~kHitBit) - 1;
            const int32_t u = par >= 0 ? link[par] : 0;    // the parent's word: its hit so far and where its chain goes on
            link[i] = (w & kHitBit) | u;
            wave_lds_sync();
        }
    }
#pragma unroll 1
    for (int c = 0; c < C; ++c) {                          // slots k .. 64 C - 1 hold INT_MAX, which is below no element
        const int i = c * 64 + lane;
        const int t = val[i];
        val[i] = i < k ? (link[i] < 0 ? base + i : t) : 0x7fffffff;
    }
    wave_lds_sync();
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const int i = c * 64 + lane, e = val[i];
        int rank = 0;                                      // ascending order: rank among the k distinct positions
#pragma unroll 2
        for (int g = 0; g < C * 16; ++g) {
            const int4 x = val4[g];
            rank += (x.x < e) + (x.y < e) + (x.z < e) + (x.w < e);
        }
        if (i < k) put(a, off + rank, p0 + e);
    }
}

__global__ __launch_bounds__(kBlock) void relabel_kernel(int32_t *__restrict__ col, const int32_t *__restrict__ map,
                                                         Counters ctr, int h)
{
    if (ctr.status()) return;
    const int e0 = ctr.edges(h), e1 = ctr.edges(h + 1);
    for (int s = e0 + blockIdx.x * kBlock + threadIdx.x; s < e1; s += gridDim.x * kBlock) col[s] = -map[col[s]] - 1;
}

// row pointer of the nodes new at the last hop (empty rows) and the end of the CSR
__global__ __launch_bounds__(kBlock) void tail_kernel(int32_t *__restrict__ out_rowPtr, Counters ctr, int64_t max_nodes)
{
    if (ctr.status()) return;
    const int H = ctr.H;
    const int i0 = ctr.nodes(H - 1), i1 = ctr.nodes(H);
    for (int i = i0 + blockIdx.x * kBlock + threadIdx.x; i <= i1 && i <= max_nodes; i += gridDim.x * kBlock)
        out_rowPtr[i] = ctr.edges(H);
}

__global__ __launch_bounds__(kBlock) void reset_kernel(const int32_t *__restrict__ n_id, int B, int n_nodes,
                                                       int32_t *__restrict__ map, Counters ctr, int64_t max_nodes)
{
    const int st = ctr.status();
    int n = st == 0 ? ctr.nodes(ctr.H) : st == kStatusSeeds ? B : 0;
    if (n > max_nodes) n = (int)max_nodes;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int v = n_id[i];
        if (v >= 0 && v < n_nodes) map[v] = kSentinel;
    }
}

}  // namespace

int sgx_sample::sample_enqueue(const int32_t *rowPtr, const int32_t *columnIndex, int n_nodes, const int32_t *seeds, int batch,
                               int n_hops, const int *fanouts, uint64_t seed, uint64_t step, const uint64_t *step_dev,
                               int32_t *node_map, int32_t *n_id, int32_t *out_rowPtr, int32_t *out_col, int32_t *edge_pos,
                               int64_t max_nodes, int64_t max_edges, const Bounds &b, int32_t *cbuf, int32_t *bsum, hipStream_t s)
{
    const Counters ctr{cbuf, n_hops};
    if (step_dev) {
        // the recorded call clears the counters with a kernel node, not a memset node: replayed after a plan build between
        // two replays (its stream-ordered allocations and frees), the memset node of the instantiated graph was seen to leave
        // the block as the previous replay had left it, and every kernel behind it then read a set status
        hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(kBlock), 0, s, cbuf, counter_count(n_hops));
    } else {
        SGX_HIP_CHECK(hipMemsetAsync(cbuf, 0, sizeof(int32_t) * counter_count(n_hops), s));
    }
    hipLaunchKernelGGL(seed_kernel, dim3(grid_of(batch, kBlock, 0)), dim3(kBlock), 0, s, seeds, batch, n_nodes, node_map,
                       n_id, ctr);
    SGX_LAUNCH_CHECK();
    for (int h = 0; h < n_hops; ++h) {
        const uint64_t key = mix64(mix64(mix64(seed) ^ step) ^ (uint64_t)h);
        scan_launch(RowCounts{ctr, rowPtr, n_id, out_rowPtr, h, fanouts[h]}, b.front[h], bsum, s);
        const SampleArgs sa{rowPtr, columnIndex, n_id, out_rowPtr, out_col, edge_pos, node_map, max_edges, key, step_dev, mix64(seed),
                            h, fanouts[h]};
        // the fan-out is uniform over the hop: its form is chosen here, through the function that reports it
        hipLaunchKernelGGL(sgx_sample_form(fanouts[h]) == 2 ? sample_wide_kernel : sample_kernel,
                           dim3(grid_of(b.front[h], kBlock / 64, 0)), dim3(kBlock), 0, s, sa, ctr);
        scan_launch(FirstSeen{ctr, out_col, node_map, n_id, max_nodes, h}, b.edges[h], bsum, s);
        hipLaunchKernelGGL(relabel_kernel, dim3(grid_of(b.edges[h], kBlock, 2048)), dim3(kBlock), 0, s, out_col, node_map,
                           ctr, h);
        SGX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tail_kernel, dim3(grid_of(b.front[n_hops - 1] + b.edges[n_hops - 1] + 1, kBlock, 2048)), dim3(kBlock),
                       0, s, out_rowPtr, ctr, max_nodes);
    hipLaunchKernelGGL(reset_kernel, dim3(grid_of(b.max_nodes, kBlock, 2048)), dim3(kBlock), 0, s, n_id, batch, n_nodes,
                       node_map, ctr, max_nodes);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

int sgx_sample::sample_finish(const int32_t *cbuf, int n_hops, int64_t *hop_nodes, int64_t *hop_edges, int32_t *extras,
                              hipStream_t s)
{
    // the one read-back of the call: status, the counts of every hop, and what a batch preparation left behind them
    int32_t host[2 * 64 + 3 + kExtras];
    SGX_HIP_CHECK(hipMemcpyAsync(host, cbuf, sizeof(int32_t) * counter_count(n_hops), hipMemcpyDeviceToHost, s));
    SGX_HIP_CHECK(hipStreamSynchronize(s));
    if (host[0] & kStatusSeeds) return SGX_ERR_SEEDS;
    if (host[0]) return SGX_ERR_SHAPE;
    for (int h = 0; h <= n_hops; ++h) {
        hop_nodes[h] = host[1 + h];
        hop_edges[h] = host[2 + n_hops + h];
    }
    if (extras)
        for (int k = 0; k < kExtras; ++k) extras[k] = host[3 + 2 * n_hops + k];
    return SGX_OK;
}

extern "C" int sgx_sample_wide_max(void) { return kWideMax; }

extern "C" int sgx_sample_form(int fanout)
{
    if (fanout < -1) return SGX_ERR_SHAPE;
    return fanout < 0 ? 0 : fanout <= kFast ? 1 : fanout <= kWideMax ? 2 : 3;
}

extern "C" size_t sgx_sample_workspace_bytes(int n_nodes, int64_t nnz, int batch, int n_hops, const int *fanouts,
                                             int64_t *max_nodes, int64_t *max_edges)
{
    Bounds b;
    if (!bounds(n_nodes, nnz, batch, n_hops, fanouts, &b)) return 0;
    if (max_nodes) *max_nodes = b.max_nodes;
    if (max_edges) *max_edges = b.max_edges;
    return counters_bytes(n_hops) + sgx_align_up(sizeof(int32_t) * b.max_tiles, 256);
}

extern "C" int sgx_sample_neighbors(const int32_t *rowPtr, const int32_t *columnIndex, int n_nodes, int64_t nnz,
                                    const int32_t *seeds, int batch, int n_hops, const int *fanouts, uint64_t seed,
                                    uint64_t step, int32_t *node_map, int32_t *n_id, int32_t *out_rowPtr,
                                    int32_t *out_col, int32_t *edge_pos, int64_t max_nodes, int64_t max_edges,
                                    int64_t *hop_nodes, int64_t *hop_edges, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    if (!fanouts || !hop_nodes || !hop_edges) return SGX_ERR_NULL;
    Bounds b;
    if (!bounds(n_nodes, nnz, batch, n_hops, fanouts, &b)) return SGX_ERR_SHAPE;
    if (max_nodes < b.max_nodes || max_edges < b.max_edges) return SGX_ERR_SHAPE;
    if (!rowPtr || !columnIndex || !node_map || !n_id || !out_rowPtr || !out_col || !edge_pos || (batch > 0 && !seeds))
        return SGX_ERR_NULL;
    if (!workspace || workspace_bytes < sgx_sample_workspace_bytes(n_nodes, nnz, batch, n_hops, fanouts, nullptr, nullptr))
        return SGX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    for (int h = 0; h <= n_hops; ++h) hop_nodes[h] = hop_edges[h] = 0;
    if (batch == 0) {
        SGX_HIP_CHECK(hipMemsetAsync(out_rowPtr, 0, sizeof(int32_t), s));
        return SGX_OK;
    }
    int32_t *cbuf = (int32_t *)workspace;
    int32_t *bsum = (int32_t *)((char *)workspace + counters_bytes(n_hops));
    const int st = sample_enqueue(rowPtr, columnIndex, n_nodes, seeds, batch, n_hops, fanouts, seed, step, nullptr, node_map, n_id,
                                  out_rowPtr, out_col, edge_pos, max_nodes, max_edges, b, cbuf, bsum, s);
    if (st != SGX_OK) return st;
    return sample_finish(cbuf, n_hops, hop_nodes, hop_edges, nullptr, s);
}
