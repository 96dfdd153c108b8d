// Neighbour sampling for mini-batch training: the NeighborLoader call pattern of the reference's demo
// (demo/emulation/demo_sgrace.py:112-125, `full_graph = 0`).  The rule -- Floyd's k-subset per frontier row, the
// counter-based draw, the relabel order -- is written down in include/sgx.h; this file is its device form.
//
// One hop is eight launches, each reading the sizes it needs from the counter block in the workspace (so nothing is
// read back between hops; every grid is sized on the host from the bound):
//   1-3  row counts of the frontier -> exclusive scan -> out_rowPtr of the frontier rows     (scan_*<RowCounts>)
//   4    one wavefront per frontier row: Floyd's subset, positions in ascending order, global column ids,
//        atomicMin of each slot's ordinal into node_map[column]                              (sample_kernel)
//   5-7  first-appearance flags (node_map[column] == own slot) -> exclusive scan -> new local ids; the first slot of a
//        node writes n_id and stores -(id + 1) in node_map                                   (scan_*<FirstSeen>)
//   8    columns relabelled through node_map                                                 (relabel_kernel)
// Kernel boundaries are the only ordering between workgroups.  A tail writes the row pointer of the last hop's new
// nodes, and the map entries of every node of n_id are put back to the sentinel.
#include "sgx_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPer = 8;                       // items per thread of a scan workgroup (contiguous)
constexpr int kTile = kBlock * kPer;          // items per scan workgroup
constexpr int kScanTop = 1024;                // threads of the one workgroup that scans the workgroup sums
constexpr int kFast = 64;                     // fan-outs up to this keep the subset in registers, one element per lane
constexpr int32_t kSentinel = 0x7fffffff;
constexpr int kStatusSeeds = 1, kStatusCapacity = 2;

// counter block: [0] status, then nodes(0..H), then edges(0..H)
struct Counters {
    int32_t *c;
    int H;
    __device__ int32_t &status() const { return c[0]; }
    __device__ int32_t &nodes(int h) const { return c[1 + h]; }
    __device__ int32_t &edges(int h) const { return c[2 + H + h]; }
    __device__ int frontier_begin(int h) const { return h ? c[h] : 0; }
};

__host__ __device__ inline uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ inline int draw(uint64_t key, int v, int j)
{
    const uint64_t w = ((uint64_t)(uint32_t)v << 32) | (uint32_t)j;
    return (int)__umul64hi(mix64(key ^ mix64(w)), (uint64_t)j + 1);     // in [0, j]
}

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
    uint64_t key;
    int h, k;
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
        const int t = lane < k ? draw(a.key, v, j) : -1;
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
            const int j = deg - k + i, t = draw(a.key, v, j);
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

// the sizes of every hop, from the fan-outs alone (sgx.h): frontier rows, sampled edges; totals
struct Bounds {
    int64_t front[64], edges[64], max_nodes, max_edges, max_tiles;
};

bool bounds(int n_nodes, int64_t nnz, int B, int n_hops, const int *fanouts, Bounds *b)
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

size_t counters_bytes(int n_hops) { return sgx_align_up(sizeof(int32_t) * (2 * n_hops + 3), 256); }

unsigned grid_of(int64_t items, int per, int64_t cap)
{
    int64_t g = (items + per - 1) / per;
    if (g < 1) g = 1;
    if (cap > 0 && g > cap) g = cap;
    return (unsigned)g;
}

}  // namespace

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
    const Counters ctr{cbuf, n_hops};
    SGX_HIP_CHECK(hipMemsetAsync(cbuf, 0, sizeof(int32_t) * (2 * n_hops + 3), s));
    hipLaunchKernelGGL(seed_kernel, dim3(grid_of(batch, kBlock, 0)), dim3(kBlock), 0, s, seeds, batch, n_nodes, node_map,
                       n_id, ctr);
    SGX_LAUNCH_CHECK();
    for (int h = 0; h < n_hops; ++h) {
        const uint64_t key = mix64(mix64(mix64(seed) ^ step) ^ (uint64_t)h);
        const RowCounts rc{ctr, rowPtr, n_id, out_rowPtr, h, fanouts[h]};
        const unsigned gr = grid_of(b.front[h], kTile, 0);
        hipLaunchKernelGGL(scan_reduce_kernel<RowCounts>, dim3(gr), dim3(kBlock), 0, s, rc, bsum);
        hipLaunchKernelGGL(scan_top_kernel<RowCounts>, dim3(1), dim3(kScanTop), 0, s, rc, bsum);
        hipLaunchKernelGGL(scan_emit_kernel<RowCounts>, dim3(gr), dim3(kBlock), 0, s, rc, bsum);
        const SampleArgs sa{rowPtr, columnIndex, n_id, out_rowPtr, out_col, edge_pos, node_map, max_edges, key, h, fanouts[h]};
        hipLaunchKernelGGL(sample_kernel, dim3(grid_of(b.front[h], kBlock / 64, 0)), dim3(kBlock), 0, s, sa, ctr);
        const FirstSeen fs{ctr, out_col, node_map, n_id, max_nodes, h};
        const unsigned ge = grid_of(b.edges[h], kTile, 0);
        hipLaunchKernelGGL(scan_reduce_kernel<FirstSeen>, dim3(ge), dim3(kBlock), 0, s, fs, bsum);
        hipLaunchKernelGGL(scan_top_kernel<FirstSeen>, dim3(1), dim3(kScanTop), 0, s, fs, bsum);
        hipLaunchKernelGGL(scan_emit_kernel<FirstSeen>, dim3(ge), dim3(kBlock), 0, s, fs, bsum);
        hipLaunchKernelGGL(relabel_kernel, dim3(grid_of(b.edges[h], kBlock, 2048)), dim3(kBlock), 0, s, out_col, node_map,
                           ctr, h);
        SGX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tail_kernel, dim3(grid_of(b.front[n_hops - 1] + b.edges[n_hops - 1] + 1, kBlock, 2048)), dim3(kBlock),
                       0, s, out_rowPtr, ctr, max_nodes);
    hipLaunchKernelGGL(reset_kernel, dim3(grid_of(b.max_nodes, kBlock, 2048)), dim3(kBlock), 0, s, n_id, batch, n_nodes,
                       node_map, ctr, max_nodes);
    SGX_LAUNCH_CHECK();
    // the one read-back of the call: status and the counts of every hop
    int32_t host[2 * 64 + 3];
    SGX_HIP_CHECK(hipMemcpyAsync(host, cbuf, sizeof(int32_t) * (2 * n_hops + 3), hipMemcpyDeviceToHost, s));
    SGX_HIP_CHECK(hipStreamSynchronize(s));
    if (host[0] & kStatusSeeds) return SGX_ERR_SEEDS;
    if (host[0]) return SGX_ERR_SHAPE;
    for (int h = 0; h <= n_hops; ++h) {
        hop_nodes[h] = host[1 + h];
        hop_edges[h] = host[2 + n_hops + h];
    }
    return SGX_OK;
}
