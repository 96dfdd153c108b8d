// A neighbour-sampled batch made layer-ready right behind the sample (include/sgx.h, "layer-ready node batches"): the
// symmetric normalisation of the sampled CSR with its self loops (sgrace.sym_norm2 + the CSR the layer reads), the rows
// n_id of the feature CSR, the labels and masks of the sampled nodes.  The launches read their sizes from the sampler's
// counter block, so nothing is read back between them and the sampler; the counts the host needs ride the sampler's
// read-back.
//   1     a wavefront per sampled row: "holds no self loop" flag, both edge lists            (loops_kernel)
//   2-4   exclusive scan of the flags -> rowPtr of the normalised matrix                     (scan_*<LoopMissing>)
//   5     rows ordered by column, the loop put in; deg and 1 / sqrt(deg) of every row        (order_kernel)
//   6     values dis[r] * w * dis[c], dead-row mask, "some row is dead", the longest row     (values_kernel)
//         sgx_node_batch_sample_quant: in the same pass the values on the unsigned w_qbits grid of one or two
//         constant sets, their dead-row masks and flags, and the lean form's mask values
//   7-9   exclusive scan of the lengths of the feature rows n_id -> rowPtr                   (scan_*<FeatureRows>)
//   10    those rows' columns and values copied; y and the masks gathered                    (gather_kernel)
// Kernel boundaries are the only ordering between workgroups.
#include "sample_device.h"
#include "quant_device.h"

using namespace sgx_sample;

namespace {

constexpr int kWaves = kBlock / 64;           // rows of one workgroup pass
constexpr int kOwn = 4;                       // long rows: entries ranked per thread and pass
constexpr int kKeys = 2048;                   // long rows: keys of one LDS tile (16 KiB)

struct Args {
    Counters ctr;
    sgx_node_batch b;
    int32_t *miss;                            // [max_nodes] 1 = the row holds no self loop
    float *dis, *w;                           // [max_nodes] 1 / sqrt(deg); [max_edges + max_nodes] weights in stored order
    __device__ int N() const { return ctr.nodes(ctr.H); }
    __device__ int E() const { return ctr.edges(ctr.H); }
};

__global__ __launch_bounds__(kBlock) void loops_kernel(Args a)
{
    if (a.ctr.status()) return;
    const int N = a.N(), lane = threadIdx.x & 63;
    const int64_t E = a.E();
    for (int r = blockIdx.x * kWaves + (threadIdx.x >> 6); r < N; r += gridDim.x * kWaves) {
        const int p0 = a.b.out_rowPtr[r], p1 = a.b.out_rowPtr[r + 1];
        bool found = false;
        for (int p = p0 + lane; p < p1; p += 64) {
            const int c = a.b.out_col[p];
            found |= c == r;
            if (a.b.edge_index_agg) {
                a.b.edge_index_agg[p] = r;
                a.b.edge_index_agg[E + p] = c;
            }
            if (a.b.edge_index) {
                a.b.edge_index[p] = c;
                a.b.edge_index[E + p] = r;
            }
        }
        const bool any = __ballot(found) != 0;
        if (lane == 0) a.miss[r] = !any;
    }
}

// items: the sampled rows; value: 1 where the row gets a loop
struct LoopMissing {
    Counters ctr;
    const int32_t *miss, *rowPtr;
    int32_t *out;
    __device__ int n() const { return ctr.nodes(ctr.H); }
    __device__ int value(int i) const { return miss[i]; }
    __device__ void emit(int i, int excl, int) const { out[i] = rowPtr[i] + excl; }
    __device__ void total(int t) const
    {
        const int nnz = ctr.edges(ctr.H) + t;
        out[n()] = nnz;
        ctr.extra(kNormNnz) = nnz;
    }
};

// items: the sampled nodes; value: the stored entries of the node's feature row
struct FeatureRows {
    Counters ctr;
    const int32_t *n_id, *rowPtr_x;
    int32_t *out;
    int64_t capacity;
    __device__ int n() const { return ctr.nodes(ctr.H); }
    __device__ int value(int i) const
    {
        const int v = n_id[i];
        return rowPtr_x[v + 1] - rowPtr_x[v];
    }
    __device__ void emit(int i, int excl, int) const { out[i] = excl; }
    __device__ void total(int t) const
    {
        out[n()] = t;
        ctr.extra(kFeaNnz) = t;
        if (t > capacity) atomicOr(&ctr.status(), kStatusCapacity);
    }
};

__device__ inline float inv_sqrt(float deg)
{
    // IEEE: the square root and the division are the correctly rounded ones (sgx.h)
    return deg > 0.0f ? 1.0f / sqrtf(deg) : 0.0f;
}

// entry j of row r in sampled order, j == len being the added loop
struct RowSource {
    const int32_t *col, *pos;
    const float *weight;
    float fill;
    int p0, len, r;
    __device__ int column(int j) const { return j < len ? col[p0 + j] : r; }
    __device__ float value(int j) const { return j < len ? (weight ? weight[pos[p0 + j]] : 1.0f) : fill; }
};

__global__ __launch_bounds__(kBlock) void order_kernel(Args a)
{
    __shared__ unsigned long long tile[kKeys];
    if (a.ctr.status()) return;
    const int N = a.N(), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const sgx_node_batch &b = a.b;
    for (int base = blockIdx.x * kWaves; base < N; base += gridDim.x * kWaves) {       // uniform over the workgroup
        // rows of up to 64 entries: one wavefront each, an entry per lane, ranks counted over shuffles
        const int r = base + wave;
        if (r < N) {
            const int p0 = b.out_rowPtr[r], q0 = b.rowPtr_norm[r];
            const int len = b.out_rowPtr[r + 1] - p0, T = b.rowPtr_norm[r + 1] - q0;
            if (T <= 64) {
                const RowSource src{b.out_col, b.edge_pos, b.edge_weight, b.fill, p0, len, r};
                const int c = lane < T ? src.column(lane) : 0x7fffffff;
                const float w = lane < T ? src.value(lane) : 0.0f;
                int rank = 0;
                for (int l = 0; l < T; ++l) {
                    const int cl = __shfl(c, l, 64);
                    rank += (cl < c) | ((cl == c) & (l < lane));
                }
                if (lane < T) {
                    b.columnIndex_norm[q0 + rank] = c;
                    a.w[q0 + rank] = w;
                }
                float deg = 0.0f;                          // the weights added one by one in stored order
                for (int k = 0; k < T; ++k) {
                    const unsigned long long at = __ballot(lane < T && rank == k);
                    deg += __shfl(w, __ffsll((long long)at) - 1, 64);
                }
                if (lane == 0) a.dis[r] = inv_sqrt(deg);
            }
        }
        // longer rows: the whole workgroup, the row's keys (column, position) streamed through LDS; any length
        for (int i = 0; i < kWaves; ++i) {
            const int rr = base + i;
            if (rr >= N) break;
            const int p0 = b.out_rowPtr[rr], q0 = b.rowPtr_norm[rr];
            const int len = b.out_rowPtr[rr + 1] - p0, T = b.rowPtr_norm[rr + 1] - q0;
            if (T <= 64) continue;                         // uniform over the workgroup
            const RowSource src{b.out_col, b.edge_pos, b.edge_weight, b.fill, p0, len, rr};
            for (int j0 = 0; j0 < T; j0 += kBlock * kOwn) {
                unsigned long long key[kOwn];
                int rank[kOwn];
#pragma unroll
                for (int u = 0; u < kOwn; ++u) {
                    const int j = j0 + u * kBlock + (int)threadIdx.x;
                    key[u] = j < T ? ((unsigned long long)(unsigned)src.column(j) << 32) | (unsigned)j : 0ull;
                    rank[u] = 0;
                }
                for (int t0 = 0; t0 < T; t0 += kKeys) {
                    const int cnt = T - t0 < kKeys ? T - t0 : kKeys;
                    __syncthreads();
                    for (int k = threadIdx.x; k < cnt; k += kBlock)
                        tile[k] = ((unsigned long long)(unsigned)src.column(t0 + k) << 32) | (unsigned)(t0 + k);
                    __syncthreads();
                    for (int k = 0; k < cnt; ++k) {
                        const unsigned long long other = tile[k];
#pragma unroll
                        for (int u = 0; u < kOwn; ++u) rank[u] += other < key[u];
                    }
                }
#pragma unroll
                for (int u = 0; u < kOwn; ++u) {
                    const int j = j0 + u * kBlock + (int)threadIdx.x;
                    if (j < T) {
                        b.columnIndex_norm[q0 + rank[u]] = (int)(key[u] >> 32);
                        a.w[q0 + rank[u]] = src.value(j);
                    }
                }
            }
            // deg: one thread adds the weights in stored order, fed through LDS
            float *ftile = (float *)tile;
            float deg = 0.0f;
            for (int t0 = 0; t0 < T; t0 += 2 * kKeys) {
                const int cnt = T - t0 < 2 * kKeys ? T - t0 : 2 * kKeys;
                __threadfence();
                __syncthreads();
                for (int k = threadIdx.x; k < cnt; k += kBlock) ftile[k] = a.w[q0 + t0 + k];
                __syncthreads();
                if (threadIdx.x == 0)
                    for (int k = 0; k < cnt; ++k) deg += ftile[k];
            }
            if (threadIdx.x == 0) a.dis[rr] = inv_sqrt(deg);
            __syncthreads();
        }
    }
}

// the NQ constant sets of sgx_node_batch_quant as the values pass takes them; NQ = 0: sgx_node_batch_sample, nothing of it
template <int NQ>
struct QuantSets {
    int qbits;
    float inv_scale[NQ], zero[NQ];
    float *val[NQ], *lean[NQ];
    uint8_t *dead[NQ];
};
template <>
struct QuantSets<0> {};

// bit 0 of the kDeadRows counter: some row of values_norm is dead; bit 1 + k: some row of constant set k is
template <class T, int NQ>
__global__ __launch_bounds__(kBlock) void values_kernel(Args a, QuantSets<NQ> qs)
{
    if (a.ctr.status()) return;
    const int N = a.N(), lane = threadIdx.x & 63;
    const sgx_node_batch &b = a.b;
    T *val = (T *)b.values_norm;
    for (int r = blockIdx.x * kWaves + (threadIdx.x >> 6); r < N; r += gridDim.x * kWaves) {
        const int q0 = b.rowPtr_norm[r], q1 = b.rowPtr_norm[r + 1];
        const float dr = a.dis[r];
        bool live = false, live_q[NQ ? NQ : 1] = {};
        for (int q = q0 + lane; q < q1; q += 64) {
            const float left = dr * a.w[q];                // (dis[r] * w) * dis[c]: two products, each rounded to fp32
            const T v = (T)(left * a.dis[b.columnIndex_norm[q]]);
            val[q] = v;
            live |= (float)v > 0.0f;
            if constexpr (NQ > 0) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) {
                    const float vq = sgx_quantizer::fake_quantize_value(0, qs.qbits, qs.inv_scale[k], qs.zero[k], (float)v);
                    qs.val[k][q] = vq;
                    live_q[k] |= vq > 0.0f;
                }
            }
        }
        int dead = __ballot(live) == 0;                    // uniform over the wavefront
        if constexpr (NQ > 0) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const bool dead_q = __ballot(live_q[k]) == 0;
                dead |= (int)dead_q << (1 + k);
                if (lane == 0) qs.dead[k][r] = dead_q;
                // the lean form's mask: a dead row keeps its unquantised values; every lane reads back its own stores
                if (qs.lean[k])
                    for (int q = q0 + lane; q < q1; q += 64) qs.lean[k][q] = dead_q ? (float)val[q] : qs.val[k][q];
            }
        }
        if (lane == 0) {
            b.dead_row[r] = dead & 1;
            // both counters are looked at first: hundreds of thousands of rows on one address serialise in L2 otherwise
            if (dead & ~__atomic_load_n(&a.ctr.extra(kDeadRows), __ATOMIC_RELAXED)) atomicOr(&a.ctr.extra(kDeadRows), dead);
            if (q1 - q0 > __atomic_load_n(&a.ctr.extra(kMaxRow), __ATOMIC_RELAXED)) atomicMax(&a.ctr.extra(kMaxRow), q1 - q0);
        }
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void gather_kernel(Args a)
{
    if (a.ctr.status()) return;
    const int N = a.N(), lane = threadIdx.x & 63;
    const sgx_node_batch &b = a.b;
    T *val = (T *)b.values_fea;
    for (int i = blockIdx.x * kWaves + (threadIdx.x >> 6); i < N; i += gridDim.x * kWaves) {
        const int v = b.n_id[i];
        if (lane == 0) {
            if (b.y) b.y_out[i] = b.y[v];
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if (b.mask[m]) b.mask_out[m][i] = b.mask[m][v];
        }
        if (!b.rowPtr_x) continue;
        const int s0 = b.rowPtr_x[v], d0 = b.rowPtr_fea[i], len = b.rowPtr_fea[i + 1] - d0;
        for (int k = lane; k < len; k += 64) {
            b.columnIndex_fea[d0 + k] = b.columnIndex_x[s0 + k];
            val[d0 + k] = (T)b.values_x[s0 + k];
        }
    }
}

size_t region(size_t bytes) { return sgx_align_up(bytes, 256); }

}  // namespace

extern "C" size_t sgx_node_batch_workspace_bytes(int n_nodes, int64_t nnz, int batch, int n_hops, const int *fanouts,
                                                 int64_t *max_nodes, int64_t *max_edges)
{
    Bounds bd;
    if (!bounds(n_nodes, nnz, batch, n_hops, fanouts, &bd)) return 0;
    if (max_nodes) *max_nodes = bd.max_nodes;
    if (max_edges) *max_edges = bd.max_edges;
    const int64_t tiles = bd.max_tiles > bd.max_nodes / kTile + 1 ? bd.max_tiles : bd.max_nodes / kTile + 1;
    return counters_bytes(n_hops) + region(sizeof(int32_t) * tiles) + 2 * region(sizeof(int32_t) * (bd.max_nodes + 1)) +
           region(sizeof(float) * (bd.max_edges + bd.max_nodes + 1));
}

namespace {

template <int NQ>
QuantSets<NQ> quant_sets(const sgx_node_batch_quant *q)
{
    QuantSets<NQ> qs{};
    if constexpr (NQ > 0) {
        qs.qbits = q->qbits;
        for (int k = 0; k < NQ; ++k) {
            qs.inv_scale[k] = q->inv_scale_adj[k];
            qs.zero[k] = q->zero_adj[k];
            qs.val[k] = q->values_q[k];
            qs.lean[k] = q->values_lean[k];
            qs.dead[k] = q->dead_row_q[k];
        }
    }
    return qs;
}

// sgx_node_batch_sample (q == NULL) and sgx_node_batch_sample_quant on their checked quantiser arguments
int node_batch_sample(sgx_node_batch *b, sgx_node_batch_quant *q, void *stream)
{
    if (!b->fanouts || !b->hop_nodes || !b->hop_edges) return SGX_ERR_NULL;
    Bounds bd;
    if (!bounds(b->n_nodes, b->nnz, b->batch, b->n_hops, b->fanouts, &bd)) return SGX_ERR_SHAPE;
    if (b->max_nodes < bd.max_nodes || b->max_edges < bd.max_edges || b->fea_capacity < 0) return SGX_ERR_SHAPE;
    if (b->dtype != SGX_F16 && b->dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    if (!b->rowPtr || !b->columnIndex || !b->node_map || !b->n_id || !b->out_rowPtr || !b->out_col || !b->edge_pos ||
        (b->batch > 0 && !b->seeds) || !b->rowPtr_norm || !b->columnIndex_norm || !b->values_norm || !b->dead_row)
        return SGX_ERR_NULL;
    if (b->rowPtr_x && (!b->columnIndex_x || !b->values_x || !b->rowPtr_fea || !b->columnIndex_fea || !b->values_fea))
        return SGX_ERR_NULL;
    if (b->y && !b->y_out) return SGX_ERR_NULL;
    for (int m = 0; m < 3; ++m)
        if (b->mask[m] && !b->mask_out[m]) return SGX_ERR_NULL;
    if (!b->workspace || b->workspace_bytes < sgx_node_batch_workspace_bytes(b->n_nodes, b->nnz, b->batch, b->n_hops, b->fanouts,
                                                                             nullptr, nullptr))
        return SGX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int H = b->n_hops;
    for (int h = 0; h <= H; ++h) b->hop_nodes[h] = b->hop_edges[h] = 0;
    b->nnz_norm = b->nnz_fea = 0;
    b->has_dead_rows = b->max_row = 0;
    if (q) q->has_dead_rows_q[0] = q->has_dead_rows_q[1] = 0;
    if (b->batch == 0) {
        SGX_HIP_CHECK(hipMemsetAsync(b->out_rowPtr, 0, sizeof(int32_t), s));
        SGX_HIP_CHECK(hipMemsetAsync(b->rowPtr_norm, 0, sizeof(int32_t), s));
        if (b->rowPtr_x) SGX_HIP_CHECK(hipMemsetAsync(b->rowPtr_fea, 0, sizeof(int32_t), s));
        return SGX_OK;
    }
    char *ws = (char *)b->workspace;
    int32_t *cbuf = (int32_t *)ws;
    ws += counters_bytes(H);
    int32_t *bsum = (int32_t *)ws;
    const int64_t tiles = bd.max_tiles > bd.max_nodes / kTile + 1 ? bd.max_tiles : bd.max_nodes / kTile + 1;
    ws += region(sizeof(int32_t) * tiles);
    Args a{Counters{cbuf, H}, *b, nullptr, nullptr, nullptr};
    a.miss = (int32_t *)ws;
    ws += region(sizeof(int32_t) * (bd.max_nodes + 1));
    a.dis = (float *)ws;
    ws += region(sizeof(int32_t) * (bd.max_nodes + 1));
    a.w = (float *)ws;
    const int st = sample_enqueue(b->rowPtr, b->columnIndex, b->n_nodes, b->seeds, b->batch, H, b->fanouts, b->seed, b->step,
                                  b->node_map, b->n_id, b->out_rowPtr, b->out_col, b->edge_pos, b->max_nodes, b->max_edges, bd,
                                  cbuf, bsum, s);
    if (st != SGX_OK) return st;
    const unsigned rows = grid_of(bd.max_nodes, kWaves, 65536);
    hipLaunchKernelGGL(loops_kernel, dim3(rows), dim3(kBlock), 0, s, a);
    scan_launch(LoopMissing{a.ctr, a.miss, b->out_rowPtr, b->rowPtr_norm}, bd.max_nodes, bsum, s);
    hipLaunchKernelGGL(order_kernel, dim3(rows), dim3(kBlock), 0, s, a);
    if (q && q->n_sets == 2)
        hipLaunchKernelGGL((values_kernel<float, 2>), dim3(rows), dim3(kBlock), 0, s, a, quant_sets<2>(q));
    else if (q)
        hipLaunchKernelGGL((values_kernel<float, 1>), dim3(rows), dim3(kBlock), 0, s, a, quant_sets<1>(q));
    else if (b->dtype == SGX_F16)
        hipLaunchKernelGGL((values_kernel<f16, 0>), dim3(rows), dim3(kBlock), 0, s, a, QuantSets<0>{});
    else
        hipLaunchKernelGGL((values_kernel<float, 0>), dim3(rows), dim3(kBlock), 0, s, a, QuantSets<0>{});
    SGX_LAUNCH_CHECK();
    if (b->rowPtr_x)
        scan_launch(FeatureRows{a.ctr, b->n_id, b->rowPtr_x, b->rowPtr_fea, b->fea_capacity}, bd.max_nodes, bsum, s);
    if (b->rowPtr_x || b->y || b->mask[0] || b->mask[1] || b->mask[2]) {
        if (b->dtype == SGX_F16)
            hipLaunchKernelGGL(gather_kernel<f16>, dim3(rows), dim3(kBlock), 0, s, a);
        else
            hipLaunchKernelGGL(gather_kernel<float>, dim3(rows), dim3(kBlock), 0, s, a);
    }
    SGX_LAUNCH_CHECK();
    int32_t extras[kExtras];
    const int done = sample_finish(cbuf, H, b->hop_nodes, b->hop_edges, extras, s);
    if (done != SGX_OK) return done;
    b->nnz_norm = extras[kNormNnz];
    b->nnz_fea = extras[kFeaNnz];
    b->has_dead_rows = extras[kDeadRows] & 1;
    b->max_row = extras[kMaxRow];
    if (q)
        for (int k = 0; k < q->n_sets; ++k) q->has_dead_rows_q[k] = (extras[kDeadRows] >> (1 + k)) & 1;
    return SGX_OK;
}

}  // namespace

extern "C" int sgx_node_batch_sample(sgx_node_batch *b, void *stream)
{
    if (!b) return SGX_ERR_NULL;
    return node_batch_sample(b, nullptr, stream);
}

extern "C" int sgx_node_batch_sample_quant(sgx_node_batch *b, sgx_node_batch_quant *q, void *stream)
{
    if (!b || !q) return SGX_ERR_NULL;
    if (b->dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;   // the quantised layer works on fp32
    if (q->n_sets != 1 && q->n_sets != 2) return SGX_ERR_SHAPE;
    if (q->qbits != 8 && q->qbits != 4 && q->qbits != 2 && q->qbits != 1) return SGX_ERR_SHAPE;
    for (int k = 0; k < q->n_sets; ++k)
        if (!q->values_q[k] || !q->dead_row_q[k]) return SGX_ERR_NULL;
    return node_batch_sample(b, q, stream);
}
