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
//   11    sgx_node_batch_sample_padded only: the filler rows, the dealt spare entries and the -1 tails behind the
//         live prefix of every array, up to a fixed capacity (pad_kernel); the counts go to a device array instead
//         of the read-back, so that call is capturable
//         sgx_node_batch_sample_padded_quant: pass 6 as sgx_node_batch_sample_quant runs it, and in pass 11 the filler
//         rows' entries of every constant set's values and lean values, on the grid, and its dead-row mask
// Kernel boundaries are the only ordering between workgroups.
#include <algorithm>
#include <functional>
#include <vector>

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
    int64_t ei_stride;                        // entries of one row of the edge lists; 0: the live edge count (unpadded)
    __device__ int N() const { return ctr.nodes(ctr.H); }
    __device__ int E() const { return ctr.edges(ctr.H); }
};

__global__ __launch_bounds__(kBlock) void loops_kernel(Args a)
{
    if (a.ctr.status()) return;
    const int N = a.N(), lane = threadIdx.x & 63;
    const int64_t E = a.ei_stride ? a.ei_stride : a.E();
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

// ---- padded node batches (sgx.h): what stands behind the live prefix of every array ----
struct PadArgs {
    int32_t N;                                // rows of every padded array
    int64_t Ca, Cf, E;                        // entries of the normalised adjacency, of the features, of the edge lists
    int32_t *status, *counts;
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// bytes [lo, hi) set to the byte `pat` (0x00: zeros; 0xff: -1 in every integer type): single bytes up to the first
// and behind the last 16-byte boundary, 16 bytes a lane between them
__device__ inline void fill_bytes(void *base, int64_t lo_bytes, int64_t hi_bytes, unsigned pat, int64_t tid, int64_t nth)
{
    if (!base || hi_bytes <= lo_bytes) return;
    char *lo = (char *)base + lo_bytes, *hi = (char *)base + hi_bytes;
    char *al = (char *)(((uintptr_t)lo + 15) & ~(uintptr_t)15);
    if (al > hi) al = hi;
    char *ah = al + ((hi - al) & ~(int64_t)15);
    const unsigned w = pat * 0x01010101u;
    const u32x4 v = {w, w, w, w};
    for (int64_t i = tid; i < al - lo; i += nth) lo[i] = (char)pat;
    for (int64_t i = tid; i < (ah - al) / 16; i += nth) reinterpret_cast<u32x4 *>(al)[i] = v;
    for (int64_t i = tid; i < hi - ah; i += nth) ah[i] = (char)pat;
}

// Behind the batch's last preparation kernel.  With a set status the batch is written as one without a live row (n =
// edges = a = f = 0: filler rows only), so that whatever reads the buffers next finds a well-formed batch; every range
// below lies inside its array's capacity whatever the counters hold (the capacities are checked on the host against the
// bounds the counters cannot pass with a clear status).
// NQ > 0 (sgx_node_batch_sample_padded_quant): the same positions of every constant set's arrays as well.  The host has
// checked that the filler's 1 stays positive and its 0 stays 0 on every set's grid, so no filler row is dead under a
// quantised mask and its lean values are its quantised ones.
template <class T, int NQ>
__global__ __launch_bounds__(kBlock) void pad_kernel(Args a, PadArgs p, QuantSets<NQ> qs)
{
    const sgx_node_batch &b = a.b;
    const int st = a.ctr.status(), H = a.ctr.H;
    const int n = st ? 0 : a.N(), e = st ? 0 : a.E();
    const int na = st ? 0 : a.ctr.extra(kNormNnz), nf = (st || !b.rowPtr_x) ? 0 : a.ctr.extra(kFeaNnz);
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nth = (int64_t)gridDim.x * kBlock;
    if (tid == 0) {
        if (st) *p.status |= st;                           // (one thread, in stream order: no other writer)
        p.counts[0] = n, p.counts[1] = e, p.counts[2] = na, p.counts[3] = nf;
        for (int h = 0; h <= H; ++h) {
            p.counts[4 + h] = st ? 0 : a.ctr.nodes(h);
            p.counts[5 + H + h] = st ? 0 : a.ctr.edges(h);
        }
    }
    const int P = p.N - n;                                 // filler rows; >= the rule's F
    const int64_t Sa = p.Ca - na - P, Sf = p.Cf - nf;      // spare entries, dealt 63 / 64 to a filler row from row 0 on
    // row pointers n .. N (entry n as the preparation left it, written again where the status skipped it)
    for (int64_t j = tid; j <= P; j += nth) {
        const int64_t da = 63 * j < Sa ? 63 * j : Sa, df = 64 * j < Sf ? 64 * j : Sf;
        b.out_rowPtr[n + j] = e;
        b.rowPtr_norm[n + j] = (int32_t)(na + j + da);
        if (b.rowPtr_x) b.rowPtr_fea[n + j] = (int32_t)(nf + df);
    }
    // the filler rows' adjacency entries: rows 0 .. full-1 hold 64, row `full` 1 + Sa % 63, the rest their diagonal 1
    T *val = (T *)b.values_norm;
    const int64_t full = Sa / 63, part = 1 + Sa % 63;
    for (int64_t t = tid; t < p.Ca - na; t += nth) {
        int64_t j, k;
        if (t < 64 * full) {
            j = t >> 6, k = t & 63;
        } else {
            const int64_t u = t - 64 * full;
            j = u < part ? full : full + 1 + (u - part);
            k = u < part ? u : 0;
        }
        b.columnIndex_norm[na + t] = (int32_t)(n + j);
        val[na + t] = k == 0 ? (T)1.0f : (T)0.0f;
        if constexpr (NQ > 0) {
#pragma unroll
            for (int s = 0; s < NQ; ++s) {
                const float vq = sgx_quantizer::fake_quantize_value(0, qs.qbits, qs.inv_scale[s], qs.zero[s], k == 0 ? 1.0f : 0.0f);
                qs.val[s][na + t] = vq;
                if (qs.lean[s]) qs.lean[s][na + t] = vq;
            }
        }
    }
    // constant ranges
    fill_bytes(b.n_id, 4ll * n, 4ll * p.N, 0xff, tid, nth);
    fill_bytes(b.dead_row, n, p.N, 0, tid, nth);
    if constexpr (NQ > 0) {
#pragma unroll
        for (int s = 0; s < NQ; ++s) fill_bytes(qs.dead[s], n, p.N, 0, tid, nth);
    }
    fill_bytes(b.y_out, 8ll * n, 8ll * p.N, 0, tid, nth);
#pragma unroll
    for (int m = 0; m < 3; ++m) fill_bytes(b.mask_out[m], n, p.N, 0, tid, nth);
    if (b.rowPtr_x) {
        fill_bytes(b.columnIndex_fea, 4ll * nf, 4ll * p.Cf, 0, tid, nth);
        fill_bytes(b.values_fea, (int64_t)sizeof(T) * nf, (int64_t)sizeof(T) * p.Cf, 0, tid, nth);
    }
    fill_bytes(b.out_col, 4ll * e, 4ll * p.E, 0xff, tid, nth);
    fill_bytes(b.edge_pos, 4ll * e, 4ll * p.E, 0xff, tid, nth);
    for (int row = 0; row < 2; ++row) {
        fill_bytes(b.edge_index, 8ll * (row * p.E + e), 8ll * (row + 1) * p.E, 0xff, tid, nth);
        fill_bytes(b.edge_index_agg, 8ll * (row * p.E + e), 8ll * (row + 1) * p.E, 0xff, tid, nth);
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

// the argument checks every node-batch call shares, behind those of its host outputs
int check_batch(const sgx_node_batch *b, Bounds &bd)
{
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
    return SGX_OK;
}

// the quantiser arguments sgx_node_batch_sample_quant and the padded quantised call share
int check_quant(const sgx_node_batch *b, const sgx_node_batch_quant *q)
{
    if (b->dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;   // the quantised layer works on fp32
    if (q->n_sets != 1 && q->n_sets != 2) return SGX_ERR_SHAPE;
    if (q->qbits != 8 && q->qbits != 4 && q->qbits != 2 && q->qbits != 1) return SGX_ERR_SHAPE;
    for (int k = 0; k < q->n_sets; ++k)
        if (!q->values_q[k] || !q->dead_row_q[k]) return SGX_ERR_NULL;
    return SGX_OK;
}

// every launch of a node batch (batch >= 1) on checked arguments, nothing read back: the sampler and the preparation
// kernels.  step_dev / ei_stride: the padded call's step word and edge-list row length (NULL / 0 otherwise).
int enqueue_batch(const sgx_node_batch *b, const sgx_node_batch_quant *q, const Bounds &bd, const uint64_t *step_dev,
                  int64_t ei_stride, Args &a, hipStream_t s)
{
    const int H = b->n_hops;
    char *ws = (char *)b->workspace;
    int32_t *cbuf = (int32_t *)ws;
    ws += counters_bytes(H);
    int32_t *bsum = (int32_t *)ws;
    const int64_t tiles = bd.max_tiles > bd.max_nodes / kTile + 1 ? bd.max_tiles : bd.max_nodes / kTile + 1;
    ws += region(sizeof(int32_t) * tiles);
    a = Args{Counters{cbuf, H}, *b, nullptr, nullptr, nullptr, ei_stride};
    a.miss = (int32_t *)ws;
    ws += region(sizeof(int32_t) * (bd.max_nodes + 1));
    a.dis = (float *)ws;
    ws += region(sizeof(int32_t) * (bd.max_nodes + 1));
    a.w = (float *)ws;
    const int st = sample_enqueue(b->rowPtr, b->columnIndex, b->n_nodes, b->seeds, b->batch, H, b->fanouts, b->seed, b->step,
                                  step_dev, b->node_map, b->n_id, b->out_rowPtr, b->out_col, b->edge_pos, b->max_nodes,
                                  b->max_edges, bd, cbuf, bsum, s);
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
    return SGX_OK;
}

// sgx_node_batch_sample (q == NULL) and sgx_node_batch_sample_quant on their checked quantiser arguments
int node_batch_sample(sgx_node_batch *b, sgx_node_batch_quant *q, void *stream)
{
    if (!b->fanouts || !b->hop_nodes || !b->hop_edges) return SGX_ERR_NULL;
    Bounds bd;
    const int ok = check_batch(b, bd);
    if (ok != SGX_OK) return ok;
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
    Args a;
    const int st = enqueue_batch(b, q, bd, nullptr, 0, a, s);
    if (st != SGX_OK) return st;
    int32_t extras[kExtras];
    const int done = sample_finish(a.ctr.c, H, b->hop_nodes, b->hop_edges, extras, s);
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
    const int ok = check_quant(b, q);
    if (ok != SGX_OK) return ok;
    return node_batch_sample(b, q, stream);
}

// ---- padded node batches: the capacity rule and the capturable call (sgx.h) ----
namespace {

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the rule's conditions on capacities that need not be the rule's own: every batch within the bounds fits
bool pad_fits(const sgx_node_batch_pad *p, const Bounds &bd, bool features)
{
    const int64_t N = p->n_rows, spare = N - bd.max_nodes;
    if (N < bd.max_nodes || p->n_edges < bd.max_edges || p->nnz_norm < bd.max_edges + N || p->nnz_fea < 0) return false;
    if (p->nnz_norm > 0x7ffffffe || p->nnz_fea > 0x7ffffffe || p->n_edges > 0x3ffffffe) return false;
    if (p->nnz_norm - N > 63 * spare) return false;        // the spare adjacency entries, 63 to a filler row
    if (features && p->nnz_fea > 64 * spare) return false; // the spare feature entries, 64 to a filler row
    return true;
}

}  // namespace

extern "C" int sgx_node_batch_pad_capacity(int n_nodes, int64_t nnz, int batch, int n_hops, const int *fanouts,
                                           const int32_t *fea_row_counts, sgx_node_batch_pad *pad)
{
    if (!pad || !fanouts) return SGX_ERR_NULL;
    Bounds bd;
    if (!bounds(n_nodes, nnz, batch, n_hops, fanouts, &bd) || batch < 1) return SGX_ERR_SHAPE;
    for (int h = 0; h < n_hops; ++h)
        if (fanouts[h] < 0) return SGX_ERR_UNSUPPORTED;    // an unbounded row
    int64_t Cf = 0;
    if (fea_row_counts) {
        std::vector<int32_t> c(fea_row_counts, fea_row_counts + n_nodes);
        for (int32_t v : c)
            if (v < 0) return SGX_ERR_SHAPE;
        std::nth_element(c.begin(), c.begin() + (bd.max_nodes < n_nodes ? bd.max_nodes : n_nodes), c.end(), std::greater<int32_t>());
        for (int64_t i = 0; i < bd.max_nodes; ++i) Cf += c[i];
    }
    const int64_t F = std::max(ceil_div(bd.max_edges, 63), ceil_div(Cf, 64));
    const int64_t N = bd.max_nodes + F, Ca = bd.max_edges + N;
    if (N > 0x7ffffffe || Ca > 0x7ffffffe || Cf > 0x7ffffffe) return SGX_ERR_SHAPE;
    pad->n_rows = (int32_t)N;
    pad->nnz_norm = Ca;
    pad->nnz_fea = Cf;
    pad->n_edges = bd.max_edges;
    return SGX_OK;
}

namespace {

// sgx_node_batch_sample_padded (q == NULL) and sgx_node_batch_sample_padded_quant on their checked quantiser arguments
int node_batch_sample_padded(const sgx_node_batch *b, const sgx_node_batch_pad *pad, const sgx_node_batch_quant *q, void *stream)
{
    if (!b->fanouts) return SGX_ERR_NULL;
    sgx_node_batch c = *b;                                 // the arguments as the kernels take them; b itself is not written
    Bounds bd;
    if (!bounds(c.n_nodes, c.nnz, c.batch, c.n_hops, c.fanouts, &bd) || c.batch < 1) return SGX_ERR_SHAPE;
    for (int h = 0; h < c.n_hops; ++h)
        if (c.fanouts[h] < 0) return SGX_ERR_UNSUPPORTED;  // an unbounded row
    c.fea_capacity = pad->nnz_fea;
    const int ok = check_batch(&c, bd);
    if (ok != SGX_OK) return ok;
    if (!pad->step || !pad->status || !pad->counts) return SGX_ERR_NULL;
    if (!pad_fits(pad, bd, c.rowPtr_x != nullptr)) return SGX_ERR_SHAPE;
    c.max_nodes = bd.max_nodes;                            // the arrays hold more; the sampler is held to its bounds
    c.max_edges = bd.max_edges;
    hipStream_t s = (hipStream_t)stream;
    Args a;
    const int st = enqueue_batch(&c, q, bd, pad->step, pad->n_edges, a, s);
    if (st != SGX_OK) return st;
    const PadArgs pa{pad->n_rows, pad->nnz_norm, c.rowPtr_x ? pad->nnz_fea : 0, pad->n_edges, pad->status, pad->counts};
    const unsigned grid = grid_of(pa.N + pa.Ca + pa.Cf + 2 * pa.E, kBlock * 4, 1024);
    if (q && q->n_sets == 2)
        hipLaunchKernelGGL((pad_kernel<float, 2>), dim3(grid), dim3(kBlock), 0, s, a, pa, quant_sets<2>(q));
    else if (q)
        hipLaunchKernelGGL((pad_kernel<float, 1>), dim3(grid), dim3(kBlock), 0, s, a, pa, quant_sets<1>(q));
    else if (c.dtype == SGX_F16)
        hipLaunchKernelGGL((pad_kernel<f16, 0>), dim3(grid), dim3(kBlock), 0, s, a, pa, QuantSets<0>{});
    else
        hipLaunchKernelGGL((pad_kernel<float, 0>), dim3(grid), dim3(kBlock), 0, s, a, pa, QuantSets<0>{});
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

}  // namespace

extern "C" int sgx_node_batch_sample_padded(sgx_node_batch *b, const sgx_node_batch_pad *pad, void *stream)
{
    if (!b || !pad) return SGX_ERR_NULL;
    return node_batch_sample_padded(b, pad, nullptr, stream);
}

extern "C" int sgx_node_batch_sample_padded_quant(sgx_node_batch *b, const sgx_node_batch_pad *pad,
                                                  const sgx_node_batch_quant *q, void *stream)
{
    if (!b || !pad || !q) return SGX_ERR_NULL;
    const int ok = check_quant(b, q);
    if (ok != SGX_OK) return ok;
    // the filler rows' 1 and 0 on every set's grid, by the rule the kernels run
    for (int k = 0; k < q->n_sets; ++k)
        if (!sgx_quantizer::filler_entries_stay_inert(q->qbits, q->inv_scale_adj[k], q->zero_adj[k])) return SGX_ERR_UNSUPPORTED;
    return node_batch_sample_padded(b, pad, q, stream);
}
