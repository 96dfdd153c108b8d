// What the classifier tail's entries share, each stated once: head_loss.hip (sgx_head_loss), node_loss.hip (sgx_node_loss),
// head_eval.hip (sgx_head_eval) and node_eval.hip (sgx_node_eval); readout.hip takes the graph logit and sample.hip the hash.
// include/sgx.h promises bits across these entries (the evaluation logits are the loss head's at p = 0, a replayed step is
// the eager one): they hold because every entry runs the functions below, in the operation order written here.
//   mix64, Dropout / dropout_key / dropout_keep   the counter-based hash and the dropout rule on it
//   row_cross_entropy                             lse, the arg-max and the target's liveness of one row of logits
//   wave_class_logit                              a graph's logit by one wavefront (the head entries, the readout)
//   node_block_front                              a block of node rows up to its logits in LDS (the node entries)
//   ordered_sum                                   slots added in index order into a double (the evaluation entries)
//   the limits, head_shape_ok / node_shape_ok / row_blocks, and the node kernels' LDS bytes
// What an entry decomposes its work into, its slices or records, its reductions and its own argument checks are its file's.
#pragma once
#include "sgx_internal.h"

namespace sgx_tail {

constexpr int kBlock = 256;
constexpr int kMaxP = 1024, kMaxC = 64;                     // every entry's limits
constexpr int kMaxCP = 16384;                               // the node entries': W [C][P] is staged in LDS
constexpr int kRows = SGX_NODE_LOSS_ROWS;                   // the node entries walk blocks of kRows rows,
constexpr int kGrid = SGX_NODE_LOSS_GRID;                   // kGrid workgroups at most
static_assert(kRows <= 32 && kRows <= kBlock / 4, "a block's selection is one 32-bit word formed by wave 0");

inline bool head_shape_ok(int G, int P, int C) { return G >= 1 && P >= 1 && C >= 1 && P <= kMaxP && C <= kMaxC; }
inline bool node_shape_ok(int64_t n_rows, int P, int C)
{
    return n_rows >= 1 && P >= 1 && C >= 1 && P <= kMaxP && C <= kMaxC && C * P <= kMaxCP;
}
inline int64_t row_blocks(int64_t n_rows) { return (n_rows + kRows - 1) / kRows; }

// The node kernels' dynamic LDS: W [C][P | 1] (an odd pitch: a class per lane reads conflict-free), the block's rows
// [kRows][P] and logits [kRows][C], then the kernel's own -- node_loss: dz [kRows][C]; node_eval: a loss and a hit per row
// and the two selection words.  w_floats: C (P | 1), which no admitted shape takes past kMaxCP + kMaxC.
constexpr size_t node_front_floats(size_t w_floats, int P, int C) { return w_floats + (size_t)kRows * P + (size_t)kRows * C; }
constexpr size_t node_loss_lds(size_t w_floats, int P, int C) { return (node_front_floats(w_floats, P, C) + (size_t)kRows * C) * sizeof(float); }
constexpr size_t node_eval_lds(size_t w_floats, int P, int C) { return (node_front_floats(w_floats, P, C) + 2 * (size_t)kRows + 2) * sizeof(float); }
constexpr size_t node_loss_lds_bytes(int P, int C) { return node_loss_lds((size_t)C * (P | 1), P, C); }
constexpr size_t node_eval_lds_bytes(int P, int C) { return node_eval_lds((size_t)C * (P | 1), P, C); }
// what the kernels opt in to: the same functions with every term at its limit
constexpr size_t kNodeLossLdsMax = node_loss_lds((size_t)kMaxCP + kMaxC, kMaxP, kMaxC);
constexpr size_t kNodeEvalLdsMax = node_eval_lds((size_t)kMaxCP + kMaxC, kMaxP, kMaxC);
static_assert(kNodeLossLdsMax >= node_loss_lds_bytes(kMaxP, kMaxCP / kMaxP) && kNodeLossLdsMax >= node_loss_lds_bytes(kMaxCP / kMaxC, kMaxC) &&
                  kNodeEvalLdsMax >= node_eval_lds_bytes(kMaxP, kMaxCP / kMaxP) && kNodeEvalLdsMax >= node_eval_lds_bytes(kMaxCP / kMaxC, kMaxC) &&
                  kNodeLossLdsMax <= 160 * 1024 && kNodeEvalLdsMax <= 160 * 1024,
              "the opt-in covers the widest and the tallest W admitted, inside a CU's 160 KiB");

// the splitmix64 finaliser: the sampler's draw (include/sgx.h, "the draw") and the dropout below hash with it
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// Dropout (include/sgx.h, "the loss head"): element e of a step is kept iff the top 24 bits of mix64(key ^ e) reach
// keep_from = floor(p 2^24), and a kept element is scaled by 1 / (1 - p), formed once in fp32.
struct Dropout {
    uint32_t keep_from;
    float scale;
};
inline Dropout dropout_of(float p_drop) { return Dropout{(uint32_t)((double)p_drop * 16777216.0), 1.0f / (1.0f - p_drop)}; }
// the step's key; step_dev: the optimiser's counter on the device (added to step) or NULL
__device__ __forceinline__ uint64_t dropout_key(uint64_t seed, uint64_t step, const int64_t *step_dev)
{
    const uint64_t step_total = step + (step_dev ? (uint64_t)step_dev[0] : 0ull);
    return mix64(mix64(seed) ^ step_total);
}
__device__ __forceinline__ bool dropout_keep(uint64_t key, int64_t element, uint32_t keep_from)
{
    return (uint32_t)(mix64(key ^ (uint64_t)element) >> 40) >= keep_from;
}

// One row of logits z[C] (in LDS) against its target t, by one thread: lse = m + logf(sum_c expf(z[c] - m)) with the sums
// from 0 in class order; best = the first class of the largest logit, a NaN never winning (a NaN z[0] counts as -inf);
// live = the target names a class -- a row whose target does not has no loss, no gradient and no hit.
struct RowCe {
    float lse;
    int best;
    bool live;
};
__device__ __forceinline__ RowCe row_cross_entropy(const float *z, int C, int64_t t)
{
#pragma clang fp contract(off)
    float m = z[0];
    for (int c = 1; c < C; ++c) m = z[c] > m ? z[c] : m;
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s = s + expf(z[c] - m);
    int best = 0;
    float bv = z[0] == z[0] ? z[0] : -INFINITY;
    for (int c = 1; c < C; ++c)
        if (z[c] > bv) bv = z[c], best = c;
    return RowCe{m + logf(s), best, t >= 0 && t < C};
}

// Class c's logit of one vector x[P] by one wavefront: a lane-strided fmaf chain over j = lane, lane + 64, ..., the xor
// butterfly, and lane 0 adds the bias -- lane 0's return value is the logit.  w: row c of W.
__device__ __forceinline__ float wave_class_logit(const float *w, const float *x, int P, int lane, const float *bias, int c)
{
    float s = 0.0f;
    for (int j = lane; j < P; j += 64) s = __builtin_fmaf(w[j], x[j], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) s = s + (bias ? bias[c] : 0.0f);
    return s;
}

// The operands of a block of node rows, which both node kernels' arguments begin with
struct NodeRows {
    int64_t n_rows, n_prefix;
    int P, C, pitch_w;
    const float *H, *W, *bias;
    const uint8_t *mask;
    float *logits;                    // NULL: only the selected rows are read
};
struct NodeBlock {
    int64_t base;                     // the block's first row
    int rows_here;
    unsigned selbits, needbits;       // per row of the block: selected (i < n_prefix and mask[i]); needed (selected, or wanted for the logits)
};
// Block b of kRows rows, by the whole workgroup: wave 0 ballots the selection into sel_s[it] (it: the parity of the
// caller's iteration -- a wave may still read the last word); needbits == 0 ends it there, H unread, and the caller goes on
// to its next block.  Otherwise W into Ws (once per workgroup: w_ready), x = the needed rows of H (DROP: under dropout,
// element i P + j of the step) into xs, zeros for the others, and a thread per (row, class) forms the logit -- one fmaf
// chain over j ascending, then the bias -- into zs and, where wanted, into r.logits.  Returns behind the barrier that
// publishes zs.
template <bool DROP>
__device__ __forceinline__ NodeBlock node_block_front(const NodeRows &r, int64_t b, int it, bool &w_ready, float *Ws, float *xs,
                                                      float *zs, unsigned *sel_s, uint64_t key = 0, Dropout drop = Dropout{0u, 1.0f})
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int P = r.P, C = r.C, pitch = r.pitch_w;
    NodeBlock k;
    k.base = b * kRows;
    k.rows_here = (int)(r.n_rows - k.base < kRows ? r.n_rows - k.base : kRows);
    if (tid < 64) {
        const int64_t i = k.base + tid;
        const bool sel = tid < k.rows_here && i < r.n_prefix && (!r.mask || r.mask[i] != 0);
        const unsigned long long bal = __ballot(sel);
        if (tid == 0) sel_s[it] = (unsigned)bal;
    }
    __syncthreads();
    k.selbits = sel_s[it];
    k.needbits = r.logits ? (k.rows_here >= 32 ? 0xffffffffu : (1u << k.rows_here) - 1u) : k.selbits;
    if (k.needbits == 0) return k;
    if (!w_ready) {
        for (int e = tid; e < C * P; e += kBlock) {
            const int c = e / P, j = e - c * P;
            Ws[c * pitch + j] = r.W[e];
        }
        w_ready = true;
    }
    for (int e = tid; e < k.rows_here * P; e += kBlock) {
        const int row = e / P;
        float v = 0.0f;
        if ((k.needbits >> row) & 1u) {
            const int64_t idx = k.base * P + e;             // i * P + j
            if (DROP)
                v = dropout_keep(key, idx, drop.keep_from) ? r.H[idx] * drop.scale : 0.0f;
            else
                v = r.H[idx];                               // p_drop = 0: x == H bit for bit
        }
        xs[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < k.rows_here * C; e += kBlock) {
        const int row = e / C, c = e - row * C;
        if (!((k.needbits >> row) & 1u)) continue;
        const float *w = Ws + c * pitch, *x = xs + row * P;
        float s = 0.0f;
        for (int j = 0; j < P; ++j) s = __builtin_fmaf(w[j], x[j], s);
        s = s + (r.bias ? r.bias[c] : 0.0f);
        zs[e] = s;
        if (r.logits) r.logits[k.base * C + e] = s;
    }
    __syncthreads();
    return k;
}

// slot(0) + slot(1) + ... + slot(n - 1), added in index order into a double from 0.0: thread 0's return value.  The
// workgroup feeds thread 0 through chunk (kBlock slots in LDS) so that the loads are coalesced; the caller's barrier
// follows.
template <typename Slot, typename Index, typename Load>
__device__ __forceinline__ double ordered_sum(Index n, Slot *chunk, Load load)
{
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (Index k0 = 0; k0 < n; k0 += kBlock) {
        const int cnt = (int)(n - k0 < kBlock ? n - k0 : kBlock);
        __syncthreads();
        if (tid < cnt) chunk[tid] = load(k0 + tid);
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < cnt; ++k) sum += (double)chunk[k];
    }
    return sum;
}

}  // namespace sgx_tail
