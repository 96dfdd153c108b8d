// Shuffled graph mini-batches collated on the device (sgx_collate_graphs, sgx_collate_graphs_extras,
// sgx_collate_graphs_padded, sgx_collate_graphs_padded_quant, include/sgx.h).
//
// The dataset lives on the device in dataset order (sgx_graph_set); a batch is a list of graph ids plus the exclusive
// offsets of every graph's rows, stored edges, adjacency entries and feature entries inside the batch, which the host
// computes from its own copy of the per-graph counts.  One wavefront owns one graph of the batch and writes all of its
// pieces -- feature rows, shifted edge list, batch vector, label, graph_ptr entry, both CSRs -- so a batch is one
// launch whatever its size: at 64 MUTAG graphs (about 1 100 rows) the cost is the launch, at thousands of graphs it is
// the bytes, which are read and written once each, coalesced across the wavefront (the feature rows 16 bytes a lane
// where source and destination share their alignment).
//
// sgx_collate_graphs_padded is the same gather into buffers of one fixed capacity, in one launch of two kinds of
// workgroup: the first (graph blocks) run the per-graph gather above, a wavefront per graph, without the entries behind
// the last graph; the others (fill blocks) read the live totals from the offset arrays' last entries and write what lies
// behind them -- the filler rows in their trailing filler graphs, those end entries, and the tails up to every capacity --
// striding over the ranges together, 16 bytes a lane where the value is constant.  The two kinds write disjoint ranges.
// sgx_collate_graphs_padded_quant is that launch with the values-only extras (the quantised adjacencies) admitted: behind
// their live entries the fill blocks write the filler rows' 1 and the spare 0 as the extra's grid holds them.
#include "quant_device.h"
#include "sgx_device.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;

struct CollateArgs {
    sgx_graph_set s;
    sgx_graph_batch b;
};

// dst[0 .. n) = src[0 .. n), one wavefront; float4 body where both pointers have the same offset modulo 16 bytes
__device__ __forceinline__ void copy_f32(float *__restrict__ dst, const float *__restrict__ src, int64_t n, int lane)
{
    const uintptr_t da = (uintptr_t)dst & 15, sa = (uintptr_t)src & 15;
    if (da == sa) {
        int64_t head = (int64_t)((16 - da) & 15) / 4;
        if (head > n) head = n;
        if (lane < head) dst[lane] = src[lane];
        const int64_t n4 = (n - head) / 4;
        float4 *__restrict__ d4 = reinterpret_cast<float4 *>(dst + head);
        const float4 *__restrict__ s4 = reinterpret_cast<const float4 *>(src + head);
        for (int64_t i = lane; i < n4; i += kWave) d4[i] = s4[i];
        for (int64_t i = head + n4 * 4 + lane; i < n; i += kWave) dst[i] = src[i];
    } else {
        for (int64_t i = lane; i < n; i += kWave) dst[i] = src[i];
    }
}

// out[o + i] = rowptr[r0 + i] - rowptr[r0] + off (i < n); col / values of the graph's entries with `shift` added to
// the columns; returns nothing, writes nothing for an empty range
__device__ __forceinline__ void copy_csr(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                         const float *__restrict__ val, int r0, int n, int32_t e0, int64_t ne,
                                         int32_t *__restrict__ rowptr_out, int32_t *__restrict__ col_out, f16 *__restrict__ v16,
                                         float *__restrict__ v32, int o, int64_t off, int shift, int lane)
{
    for (int i = lane; i < n; i += kWave) rowptr_out[o + i] = (int32_t)(off + (rowptr[r0 + i] - e0));
    for (int64_t i = lane; i < ne; i += kWave) {
        const int c = col[e0 + i];
        const float v = val[e0 + i];
        col_out[off + i] = c + shift;
        if (v16) v16[off + i] = (f16)v;
        if (v32) v32[off + i] = v;
    }
}

// everything sgx_collate_graphs writes for batch position `pos`, one wavefront; false (nothing written) for a graph id
// outside the set or ranges that do not fit the totals.  kEnds: the last position also writes the entries behind the
// last graph (graph_ptr[n_graphs] and both row pointers' last); a padded batch's lie behind its filler rows instead
template <bool kEnds = true>
__device__ __forceinline__ bool collate_one(const sgx_graph_set &s, const sgx_graph_batch &b, int pos, int lane)
{
    const int g = b.index[pos];
    if (g < 0 || g >= s.n_graphs) return false;
    const int r0 = s.node_ptr[g], n = s.node_ptr[g + 1] - r0;
    const int64_t se0 = s.edge_ptr[g], ne = (int64_t)s.edge_ptr[g + 1] - se0;
    const int32_t a0 = s.rowPtr_adj[r0], f0 = s.rowPtr_fea[r0];
    const int64_t na = (int64_t)s.rowPtr_adj[r0 + n] - a0, nf = (int64_t)s.rowPtr_fea[r0 + n] - f0;
    const int o = b.node_off[pos];
    const int64_t eo = b.edge_off[pos], ao = b.adj_off[pos], fo = b.fea_off[pos];
    // offsets that do not match the set's counts: skip the graph rather than write past a buffer
    if (n < 0 || ne < 0 || na < 0 || nf < 0 || o < 0 || (int64_t)o + n > b.n_rows || eo < 0 || eo + ne > b.n_edges ||
        ao < 0 || ao + na > b.nnz_adj || fo < 0 || fo + nf > b.nnz_fea)
        return false;
    if (lane == 0) {
        b.graph_ptr[pos] = o;
        b.y[pos] = s.y[g];
        if (kEnds && pos == b.n_graphs - 1) {
            b.graph_ptr[b.n_graphs] = b.n_rows;
            b.rowPtr_adj[b.n_rows] = (int32_t)b.nnz_adj;
            b.rowPtr_fea[b.n_rows] = (int32_t)b.nnz_fea;
        }
    }
    for (int i = lane; i < n; i += kWave) b.batch[o + i] = pos;
    copy_f32(b.x + (int64_t)o * s.n_feat, s.x + (int64_t)r0 * s.n_feat, (int64_t)n * s.n_feat, lane);
    const int32_t *__restrict__ src = s.edge_index + se0, *__restrict__ dst = s.edge_index + s.n_edges + se0;
    for (int64_t i = lane; i < ne; i += kWave) {
        b.edge_index[eo + i] = (int64_t)src[i] + o;
        b.edge_index[b.n_edges + eo + i] = (int64_t)dst[i] + o;
    }
    copy_csr(s.rowPtr_adj, s.columnIndex_adj, s.values_adj, r0, n, a0, na, b.rowPtr_adj, b.columnIndex_adj,
             static_cast<f16 *>(b.values_adj[SGX_F16]), static_cast<float *>(b.values_adj[SGX_F32]), o, ao, o - r0, lane);
    copy_csr(s.rowPtr_fea, s.columnIndex_fea, s.values_fea, r0, n, f0, nf, b.rowPtr_fea, b.columnIndex_fea,
             static_cast<f16 *>(b.values_fea[SGX_F16]), static_cast<float *>(b.values_fea[SGX_F32]), o, fo, 0, lane);
    return true;
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void collate_graphs_kernel(CollateArgs a)
{
    const int lane = threadIdx.x % kWave;
    const int64_t bi = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    if (bi >= a.b.n_graphs) return;
    collate_one(a.s, a.b, (int)bi, lane);
}

struct CollateExtraArgs {
    sgx_graph_set s;
    sgx_graph_batch b;
    sgx_collate_extra x[SGX_COLLATE_MAX_EXTRAS];
    int n_extras;
};

// sgx_collate_graphs_extras: the batch as above plus, per extra, the graph's entry range of a dataset-side CSR copied as
// one contiguous, lane-strided run (a graph's rows are consecutive in the set, so its entries are too) -- columns shifted,
// values cast per dtype -- the shifted row pointer and the row bytes.  Every range of every extra is checked before the
// first store, so a graph is written as a whole or not at all.
template <bool kEnds>
__device__ __forceinline__ void collate_one_extras(const CollateExtraArgs &a, int pos, int lane)
{
    const sgx_graph_set &s = a.s;
    const sgx_graph_batch &b = a.b;
    const int g = b.index[pos];
    if (g < 0 || g >= s.n_graphs) return;
    const int r0 = s.node_ptr[g], n = s.node_ptr[g + 1] - r0;
    const int o = b.node_off[pos];
    if (n < 0 || o < 0 || (int64_t)o + n > b.n_rows) return;
    int32_t e0[SGX_COLLATE_MAX_EXTRAS];
    int64_t ne[SGX_COLLATE_MAX_EXTRAS], eo[SGX_COLLATE_MAX_EXTRAS];
#pragma unroll
    for (int k = 0; k < SGX_COLLATE_MAX_EXTRAS; ++k) {
        if (k >= a.n_extras) break;
        const sgx_collate_extra &x = a.x[k];
        e0[k] = x.rowPtr[r0];
        ne[k] = (int64_t)x.rowPtr[r0 + n] - e0[k];
        eo[k] = x.entry_off[pos];
        if (ne[k] < 0 || eo[k] < 0 || eo[k] + ne[k] > x.nnz) return;
    }
    if (!collate_one<kEnds>(s, b, pos, lane)) return;
#pragma unroll
    for (int k = 0; k < SGX_COLLATE_MAX_EXTRAS; ++k) {
        if (k >= a.n_extras) break;
        const sgx_collate_extra &x = a.x[k];
        const int64_t off = eo[k];
        if (x.rowPtr_out) {
            for (int i = lane; i < n; i += kWave) x.rowPtr_out[o + i] = (int32_t)(off + (x.rowPtr[r0 + i] - e0[k]));
            if (kEnds && lane == 0 && pos == b.n_graphs - 1) x.rowPtr_out[b.n_rows] = (int32_t)x.nnz;
            const int32_t *__restrict__ col = x.columnIndex + e0[k];
            const int shift = o - r0;
            for (int64_t i = lane; i < ne[k]; i += kWave) x.columnIndex_out[off + i] = col[i] + shift;
        }
        const float *__restrict__ val = x.values + e0[k];
        f16 *__restrict__ v16 = static_cast<f16 *>(x.values_out[SGX_F16]);
        float *__restrict__ v32 = static_cast<float *>(x.values_out[SGX_F32]);
        if (v16 || v32) {
            for (int64_t i = lane; i < ne[k]; i += kWave) {
                const float v = val[i];
                if (v16) v16[off + i] = (f16)v;
                if (v32) v32[off + i] = v;
            }
        }
        if (x.dead_row)
            for (int i = lane; i < n; i += kWave) x.dead_row_out[o + i] = x.dead_row[r0 + i];
    }
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void collate_graphs_extras_kernel(CollateExtraArgs a)
{
    const int lane = threadIdx.x % kWave;
    const int64_t bi = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    if (bi >= a.b.n_graphs) return;
    collate_one_extras<true>(a, (int)bi, lane);
}

// ---- padded batches (sgx_collate_graphs_padded, include/sgx.h "padded batches") ----------------------------------------
// The totals of a.c.b and the nnz of every extra are the CAPACITIES; the live totals are the offset arrays' last entries.
struct CollatePadArgs {
    CollateExtraArgs c;
    int G, R_f;                  // graphs with the fillers, rows of a full filler graph
    unsigned graph_blocks;       // blocks [0, graph_blocks) gather the graphs, the others write the filler rows and the tails
    sgx_collate_pad_quant q;     // the grid of every values-only extra (sgx_collate_graphs_padded_quant; unread otherwise)
};

constexpr int kFillThreads = kWave * kWavesPerBlock;

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct alignas(16) Vec16 {
    uint32_t w[4];
};

// p[lo .. hi) = v by the fill threads (t of nt >= 16): 16-byte stores over the aligned body, single elements at both ends
template <typename T>
__device__ __forceinline__ void fill_range(T *__restrict__ p, int64_t lo, int64_t hi, T v, int64_t t, int64_t nt)
{
    if (!p || lo >= hi) return;
    constexpr int kPer = 16 / (int)sizeof(T);
    T e[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) e[i] = v;
    Vec16 v16;
    __builtin_memcpy(&v16, e, 16);
    int64_t head = (int64_t)((16 - ((uintptr_t)(p + lo) & 15)) & 15) / (int64_t)sizeof(T);
    if (head > hi - lo) head = hi - lo;
    const int64_t body = (hi - lo - head) / kPer;
    if (t < head) p[lo + t] = v;
    Vec16 *__restrict__ q = reinterpret_cast<Vec16 *>(p + lo + head);
    for (int64_t i = t; i < body; i += nt) q[i] = v16;
    for (int64_t i = lo + head + body * kPer + t; i < hi; i += nt) p[i] = v;
}

// behind a CSR's live entries [0, a): one diagonal entry of value 1 per filler row n + j (j < P, as far as the capacity
// goes), zeros up to the capacity; the filler rows' pointers and the last one
__device__ __forceinline__ void fill_pattern(int32_t *__restrict__ rowptr, int32_t *__restrict__ col, f16 *__restrict__ v16,
                                             float *__restrict__ v32, int n, int N, int64_t a, int64_t cap, int64_t t, int64_t nt)
{
    const int64_t P = N - n;
    for (int64_t j = t; j <= P; j += nt) rowptr[n + j] = (int32_t)(a + j < cap ? a + j : cap);      // (j == P: rowptr[N])
    for (int64_t i = a + t; i < cap; i += nt) {
        const bool diag = i - a < P;
        col[i] = diag ? (int32_t)(n + (i - a)) : 0;
        if (v16) v16[i] = diag ? (f16)1.0f : (f16)0.0f;
        if (v32) v32[i] = diag ? 1.0f : 0.0f;
    }
}

__device__ __forceinline__ void fill_padding(const CollatePadArgs &a, int64_t t, int64_t nt)
{
    const sgx_graph_set &s = a.c.s;
    const sgx_graph_batch &b = a.c.b;
    const int B = b.n_graphs, N = b.n_rows, G = a.G, R = a.R_f;
    const int n = (int)clamp_to(b.node_off[B], N);
    const int64_t E = clamp_to(b.edge_off[B], b.n_edges), na = clamp_to(b.adj_off[B], b.nnz_adj), nf = clamp_to(b.fea_off[B], b.nnz_fea);
    const int64_t P = N - n;
    for (int64_t j = t; j < P; j += nt) {
        const int64_t g = B + (R > 0 ? j / R : 0);
        b.batch[n + j] = g < G ? g : G - 1;
        b.rowPtr_fea[n + j] = (int32_t)nf;
    }
    if (t == 0) b.rowPtr_fea[N] = (int32_t)nf;
    for (int64_t k = t; k <= G - B; k += nt) {
        const int64_t rows = k * (int64_t)R;
        b.graph_ptr[B + k] = (int32_t)(n + (rows < P ? rows : P));
        if (k < G - B) b.y[B + k] = 0;
    }
    fill_range(b.x, (int64_t)n * s.n_feat, (int64_t)N * s.n_feat, 0.0f, t, nt);
    fill_range(b.edge_index, E, b.n_edges, (int64_t)-1, t, nt);
    fill_range(b.edge_index, b.n_edges + E, 2 * b.n_edges, (int64_t)-1, t, nt);
    fill_pattern(b.rowPtr_adj, b.columnIndex_adj, static_cast<f16 *>(b.values_adj[SGX_F16]), static_cast<float *>(b.values_adj[SGX_F32]),
                 n, N, na, b.nnz_adj, t, nt);
    fill_range(b.columnIndex_fea, nf, b.nnz_fea, (int32_t)0, t, nt);
    fill_range(static_cast<f16 *>(b.values_fea[SGX_F16]), nf, b.nnz_fea, (f16)0.0f, t, nt);
    fill_range(static_cast<float *>(b.values_fea[SGX_F32]), nf, b.nnz_fea, 0.0f, t, nt);
    for (int k = 0; k < a.c.n_extras; ++k) {
        const sgx_collate_extra &x = a.c.x[k];
        if (!x.rowPtr_out) {
            // values over the pattern of an extra before it: the filler rows' diagonal 1 and the spare 0 on this extra's grid
            const float one = sgx_quantizer::fake_quantize_value(0, a.q.qbits[k], a.q.inv_scale_adj[k], a.q.zero_adj[k], 1.0f);
            const float zero = sgx_quantizer::fake_quantize_value(0, a.q.qbits[k], a.q.inv_scale_adj[k], a.q.zero_adj[k], 0.0f);
            const int64_t live = clamp_to(x.entry_off[B], x.nnz), diag = live + P < x.nnz ? live + P : x.nnz;
            fill_range(static_cast<f16 *>(x.values_out[SGX_F16]), live, diag, (f16)one, t, nt);
            fill_range(static_cast<f16 *>(x.values_out[SGX_F16]), diag, x.nnz, (f16)zero, t, nt);
            fill_range(static_cast<float *>(x.values_out[SGX_F32]), live, diag, one, t, nt);
            fill_range(static_cast<float *>(x.values_out[SGX_F32]), diag, x.nnz, zero, t, nt);
            fill_range(x.dead_row_out, (int64_t)n, (int64_t)N, (uint8_t)0, t, nt);
            continue;
        }
        fill_pattern(x.rowPtr_out, x.columnIndex_out, static_cast<f16 *>(x.values_out[SGX_F16]), static_cast<float *>(x.values_out[SGX_F32]),
                     n, N, clamp_to(x.entry_off[B], x.nnz), x.nnz, t, nt);
        fill_range(x.dead_row_out, (int64_t)n, (int64_t)N, (uint8_t)0, t, nt);
    }
}

__global__ __launch_bounds__(kFillThreads) void collate_graphs_padded_kernel(CollatePadArgs a)
{
    if (blockIdx.x < a.graph_blocks) {
        const int64_t bi = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
        if (bi < a.c.b.n_graphs) collate_one_extras<false>(a.c, (int)bi, threadIdx.x % kWave);
        return;
    }
    fill_padding(a, (int64_t)(blockIdx.x - a.graph_blocks) * kFillThreads + threadIdx.x, (int64_t)(gridDim.x - a.graph_blocks) * kFillThreads);
}

int check_collate(const sgx_graph_set *s, const sgx_graph_batch *b)
{
    if (!s || !b) return SGX_ERR_NULL;
    if (s->n_graphs < 1 || s->n_feat < 1 || s->n_edges < 0) return SGX_ERR_SHAPE;
    if (b->n_graphs < 1 || b->n_rows < 0 || b->n_edges < 0 || b->nnz_adj < 0 || b->nnz_fea < 0) return SGX_ERR_SHAPE;
    if (!s->node_ptr || !s->edge_ptr || !s->x || !s->y || !s->rowPtr_adj || !s->columnIndex_adj || !s->values_adj ||
        !s->rowPtr_fea || !s->columnIndex_fea || !s->values_fea || (s->n_edges > 0 && !s->edge_index))
        return SGX_ERR_NULL;
    if (!b->index || !b->node_off || !b->edge_off || !b->adj_off || !b->fea_off || !b->batch || !b->y || !b->graph_ptr ||
        !b->rowPtr_adj || !b->rowPtr_fea)
        return SGX_ERR_NULL;
    if ((b->n_rows > 0 && !b->x) || (b->n_edges > 0 && !b->edge_index) || (b->nnz_adj > 0 && !b->columnIndex_adj) ||
        (b->nnz_fea > 0 && !b->columnIndex_fea))
        return SGX_ERR_NULL;
    return SGX_OK;
}

int check_extras(const sgx_graph_batch *b, const sgx_collate_extra *extras, int n_extras)
{
    if (n_extras > 0 && !extras) return SGX_ERR_NULL;
    for (int k = 0; k < n_extras; ++k) {
        const sgx_collate_extra &x = extras[k];
        if (x.nnz < 0) return SGX_ERR_SHAPE;
        if (!x.rowPtr || !x.values || !x.entry_off) return SGX_ERR_NULL;
        if (!x.rowPtr_out && x.columnIndex_out) return SGX_ERR_NULL;
        if (x.rowPtr_out && (!x.columnIndex || (x.nnz > 0 && !x.columnIndex_out))) return SGX_ERR_NULL;
        if (b->n_rows > 0 && (x.dead_row == nullptr) != (x.dead_row_out == nullptr)) return SGX_ERR_NULL;
    }
    return SGX_OK;
}

}  // namespace

extern "C" int sgx_collate_graphs(const sgx_graph_set *set, const sgx_graph_batch *b, void *stream)
{
    const int rc = check_collate(set, b);
    if (rc != SGX_OK) return rc;
    CollateArgs a;
    a.s = *set;
    a.b = *b;
    const unsigned grid = (unsigned)((b->n_graphs + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(collate_graphs_kernel, dim3(grid), dim3(kWave * kWavesPerBlock), 0, (hipStream_t)stream, a);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

extern "C" int sgx_collate_graphs_extras(const sgx_graph_set *set, const sgx_graph_batch *b, const sgx_collate_extra *extras,
                                         int n_extras, void *stream)
{
    if (n_extras < 0 || n_extras > SGX_COLLATE_MAX_EXTRAS) return SGX_ERR_SHAPE;
    int rc = check_collate(set, b);
    if (rc != SGX_OK) return rc;
    rc = check_extras(b, extras, n_extras);
    if (rc != SGX_OK) return rc;
    CollateExtraArgs a = {};
    a.s = *set;
    a.b = *b;
    for (int k = 0; k < n_extras; ++k) a.x[k] = extras[k];
    a.n_extras = n_extras;
    const unsigned grid = (unsigned)((b->n_graphs + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(collate_graphs_extras_kernel, dim3(grid), dim3(kWave * kWavesPerBlock), 0, (hipStream_t)stream, a);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

namespace {

// the quantiser arguments of sgx_collate_graphs_padded_quant: every values-only extra k of x [n_extras] (capacities in place)
// has a pattern-bearing extra of its capacity before it and a grid q that keeps the filler entries inert
int check_pad_quant(const sgx_collate_extra *x, int n_extras, const sgx_collate_pad_quant *q)
{
    int pattern = -1;
    for (int k = 0; k < n_extras; ++k) {
        if (x[k].rowPtr_out) { pattern = k; continue; }
        if (!q) return SGX_ERR_NULL;
        if (pattern < 0 || x[k].nnz != x[pattern].nnz) return SGX_ERR_SHAPE;
        const int bits = q->qbits[k];
        if (bits != 8 && bits != 4 && bits != 2 && bits != 1) return SGX_ERR_UNSUPPORTED;
        if (!sgx_quantizer::filler_entries_stay_inert(bits, q->inv_scale_adj[k], q->zero_adj[k])) return SGX_ERR_UNSUPPORTED;
    }
    return SGX_OK;
}

// both padded entry points; quant: values-only extras are admitted, on the grids of q
int collate_padded(const sgx_graph_set *set, const sgx_graph_batch *b, const sgx_collate_extra *extras, int n_extras,
                   const sgx_collate_pad *pad, bool quant, const sgx_collate_pad_quant *q, void *stream)
{
    if (n_extras < 0 || n_extras > SGX_COLLATE_MAX_EXTRAS) return SGX_ERR_SHAPE;
    if (!b || !pad) return SGX_ERR_NULL;
    CollatePadArgs a = {};
    a.c.b = *b;                                   // the capacities take the totals' place: every range is tested against them
    a.c.b.n_rows = pad->n_rows;
    a.c.b.n_edges = pad->n_edges;
    a.c.b.nnz_adj = pad->nnz_adj;
    a.c.b.nnz_fea = pad->nnz_fea;
    if (n_extras > 0 && !extras) return SGX_ERR_NULL;
    for (int k = 0; k < n_extras; ++k) {
        a.c.x[k] = extras[k];
        a.c.x[k].nnz = pad->nnz_extra[k];
    }
    int rc = quant ? check_pad_quant(a.c.x, n_extras, q) : SGX_OK;
    if (rc != SGX_OK) return rc;
    rc = check_collate(set, &a.c.b);
    if (rc != SGX_OK) return rc;
    rc = check_extras(&a.c.b, a.c.x, n_extras);
    if (rc != SGX_OK) return rc;
    const int64_t B = b->n_graphs, N = pad->n_rows, G = pad->n_graphs, R = pad->filler_rows;
    // the least that every batch of B graphs of at most R rows leaves to the fillers: an entry per row in every pattern
    const int64_t least = N > B * R ? N - B * R : 0;
    if (G < B || R < 0 || G * R < N || pad->nnz_adj < least || pad->nnz_adj > INT32_MAX || pad->nnz_fea > INT32_MAX) return SGX_ERR_SHAPE;
    for (int k = 0; k < n_extras; ++k) {
        if (!a.c.x[k].rowPtr_out && !quant) return SGX_ERR_UNSUPPORTED;         // values only (the quantised adjacencies)
        if (a.c.x[k].nnz < least || a.c.x[k].nnz > INT32_MAX) return SGX_ERR_SHAPE;
    }
    if (q) a.q = *q;
    a.c.s = *set;
    a.c.n_extras = n_extras;
    a.G = (int)G;
    a.R_f = (int)R;
    a.graph_blocks = (unsigned)((B + kWavesPerBlock - 1) / kWavesPerBlock);
    // the filler rows and the tails: a block per 8 192 elements of capacity, 64 at the most
    int64_t work = N * (set->n_feat + 3) + 2 * pad->n_edges + 2 * pad->nnz_adj + 2 * pad->nnz_fea;
    for (int k = 0; k < n_extras; ++k) work += 2 * pad->nnz_extra[k];
    int64_t fill_blocks = (work + 8191) / 8192;
    fill_blocks = fill_blocks < 1 ? 1 : (fill_blocks > 64 ? 64 : fill_blocks);
    hipLaunchKernelGGL(collate_graphs_padded_kernel, dim3(a.graph_blocks + (unsigned)fill_blocks), dim3(kFillThreads), 0,
                       (hipStream_t)stream, a);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}

}  // namespace

extern "C" int sgx_collate_graphs_padded(const sgx_graph_set *set, const sgx_graph_batch *b, const sgx_collate_extra *extras,
                                         int n_extras, const sgx_collate_pad *pad, void *stream)
{
    return collate_padded(set, b, extras, n_extras, pad, false, nullptr, stream);
}

extern "C" int sgx_collate_graphs_padded_quant(const sgx_graph_set *set, const sgx_graph_batch *b, const sgx_collate_extra *extras,
                                               int n_extras, const sgx_collate_pad *pad, const sgx_collate_pad_quant *q, void *stream)
{
    return collate_padded(set, b, extras, n_extras, pad, true, q, stream);
}
