// The classifier tail of an evaluation pass over node batches in one call (sgx_node_eval, include/sgx.h "the node
// evaluation head"): the C x P Linear head on the SELECTED rows of a node matrix (a prefix, a byte mask, or both), the
// per-row cross entropy and the arg-max's hit, ADDED to accumulators that stay on the device across the batches of a pass
// -- totals[0] += selected rows, totals[1] += hits, loss_sum += the summed loss.  What demo_sgrace.py's test(loader, split)
// runs per batch as model(...), out[:batch_size], argmax, ==, sum and a read-back.
//
// Two launches, as sgx_head_eval.  The first is sgx_node_loss's main kernel without its gradients: a workgroup takes the row
// blocks b, b + grid, ... of SGX_NODE_LOSS_ROWS rows; a block none of whose rows is needed (selected, or wanted for the
// logits output) is not read; otherwise W is staged in LDS (once per workgroup), the block's rows in LDS, a thread per
// (row, class) forms the logit in sgx_node_loss's order (one fmaf chain over j ascending, then the bias), a thread per
// selected row forms lse, the loss and the arg-max exactly as sgx_node_loss does, and thread 0 adds the block's selected
// rows' losses in row order into a double and stores the block's record -- that double, the rows it selected, its hits -- in
// the block's own workspace slot.  Nothing that is summed depends on the grid.  The second, one workgroup: the records'
// integers, then their doubles added in block order, and all three added to the accumulators.  No atomics: the same bits
// on every run and for any grid.
#include "sgx_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRows = SGX_NODE_LOSS_ROWS;
constexpr int kGrid = SGX_NODE_LOSS_GRID;
constexpr int kMaxP = 1024, kMaxC = 64, kMaxCP = 16384;     // sgx_node_loss's limits
constexpr size_t kHeader = 256;                             // the workspace's first 256 bytes are reserved
static_assert(kRows <= 32 && kRows <= kBlock / 4, "a block's selection is one 32-bit word formed by wave 0");

struct BlockRecord {                  // one per block of kRows rows that can hold a selected row
    double loss;                      // its selected rows' fp32 losses, added from 0.0 in row order
    int32_t rows, hits;
};
static_assert(sizeof(BlockRecord) == 16, "the workspace rule counts 16 bytes a block");

struct NodeEvalArgs {
    int64_t n_rows, n_prefix, n_blocks, n_sel_blocks;      // blocks the first launch walks; blocks that own a record
    int P, C, pitch_w;
    const float *H, *W, *bias;
    const int64_t *target;
    const uint8_t *mask;
    int64_t *totals;
    double *loss_sum;
    float *logits;
    BlockRecord *records;             // [n_sel_blocks]
};

__global__ __launch_bounds__(kBlock) void node_eval_kernel(NodeEvalArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char node_eval_lds[];
    const int tid = threadIdx.x;
    const int P = a.P, C = a.C, CP = C * P, pitch = a.pitch_w;
    float *const Ws = reinterpret_cast<float *>(node_eval_lds);   // [C][pitch]: an odd pitch, a class per lane reads conflict-free
    float *const xs = Ws + (size_t)C * pitch;                     // [kRows][P]
    float *const zs = xs + (size_t)kRows * P;                     // [kRows][C]
    float *const loss_s = zs + (size_t)kRows * C;                 // [kRows]
    int *const hit_s = reinterpret_cast<int *>(loss_s + kRows);   // [kRows]
    unsigned *const sel_s = reinterpret_cast<unsigned *>(hit_s + kRows);   // [2], by the parity of the iteration
    bool w_ready = false;
    int it = 0;
    for (int64_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x, it ^= 1) {
        const int64_t base = b * kRows;
        const int rows_here = (int)(a.n_rows - base < kRows ? a.n_rows - base : kRows);
        if (tid < 64) {
            const int64_t i = base + tid;
            const bool sel = tid < rows_here && i < a.n_prefix && (!a.mask || a.mask[i] != 0);
            const unsigned long long bal = __ballot(sel);
            if (tid == 0) sel_s[it] = (unsigned)bal;
        }
        __syncthreads();
        const unsigned selbits = sel_s[it];
        const unsigned needbits = a.logits ? (rows_here >= 32 ? 0xffffffffu : (1u << rows_here) - 1u) : selbits;
        if (needbits == 0) {                                // nothing to compute: H is not read
            if (tid == 0 && b < a.n_sel_blocks) a.records[b] = BlockRecord{0.0, 0, 0};
            continue;
        }
        if (!w_ready) {
            for (int e = tid; e < CP; e += kBlock) {
                const int c = e / P, j = e - c * P;
                Ws[c * pitch + j] = a.W[e];
            }
            w_ready = true;
        }
        for (int e = tid; e < rows_here * P; e += kBlock) {
            const int r = e / P;
            xs[e] = ((needbits >> r) & 1u) ? a.H[base * P + e] : 0.0f;      // p_drop = 0: x == H bit for bit
        }
        __syncthreads();
        for (int e = tid; e < rows_here * C; e += kBlock) {
            const int r = e / C, c = e - r * C;
            if (!((needbits >> r) & 1u)) continue;
            const float *w = Ws + c * pitch, *x = xs + r * P;
            float s = 0.0f;
            for (int j = 0; j < P; ++j) s = __builtin_fmaf(w[j], x[j], s);
            s = s + (a.bias ? a.bias[c] : 0.0f);
            zs[e] = s;
            if (a.logits) a.logits[base * C + e] = s;
        }
        __syncthreads();
        if (tid < kRows) {
            float loss = 0.0f;
            int hit = 0;
            if ((selbits >> tid) & 1u) {
                const float *z = zs + tid * C;
                const int64_t t = a.target[base + tid];
                const bool live = t >= 0 && t < C;
                float m = z[0];
                for (int c = 1; c < C; ++c) m = z[c] > m ? z[c] : m;
                float s = 0.0f;
                for (int c = 0; c < C; ++c) s = s + expf(z[c] - m);
                const float lse = m + logf(s);
                int best = 0;
                float bv = z[0] == z[0] ? z[0] : -INFINITY;
                for (int c = 1; c < C; ++c)
                    if (z[c] > bv) bv = z[c], best = c;
                if (live) {
                    loss = lse - z[t];
                    hit = best == (int)t;
                }
            }
            loss_s[tid] = loss, hit_s[tid] = hit;
        }
        __syncthreads();
        if (tid == 0 && b < a.n_sel_blocks) {
            BlockRecord rec{0.0, 0, 0};
            for (int r = 0; r < kRows; ++r)
                if ((selbits >> r) & 1u) rec.loss += (double)loss_s[r], rec.rows += 1, rec.hits += hit_s[r];
            a.records[b] = rec;
        }
        // xs, zs, loss_s and hit_s are rewritten only behind the next iteration's first barrier or later, which thread 0
        // reaches after the loop above; sel_s alternates
    }
}

// the sums, by one workgroup: the records' integers (any order), then their doubles in block order, fed through LDS
__global__ __launch_bounds__(kBlock) void node_eval_sum_kernel(NodeEvalArgs a)
{
    __shared__ double chunk[kBlock];
    __shared__ int64_t rows_s[kBlock], hits_s[kBlock];
    const int tid = threadIdx.x;
    int64_t rows = 0, hits = 0;
    for (int64_t k = tid; k < a.n_sel_blocks; k += kBlock) rows += a.records[k].rows, hits += a.records[k].hits;
    rows_s[tid] = rows, hits_s[tid] = hits;
    double sum = 0.0;                                        // thread 0's
    for (int64_t k0 = 0; k0 < a.n_sel_blocks; k0 += kBlock) {
        const int cnt = (int)(a.n_sel_blocks - k0 < kBlock ? a.n_sel_blocks - k0 : kBlock);
        __syncthreads();
        if (tid < cnt) chunk[tid] = a.records[k0 + tid].loss;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < cnt; ++k) sum += chunk[k];
    }
    __syncthreads();
    if (tid == 0) {
        int64_t M = 0, n = 0;
        for (int k = 0; k < kBlock; ++k) M += rows_s[k], n += hits_s[k];
        if (M > 0) {                                         // nothing selected: the accumulators are not touched
            a.totals[0] += M;
            a.totals[1] += n;
            a.loss_sum[0] += sum;
        }
    }
}

bool node_eval_shape_ok(int64_t n_rows, int P, int C)
{
    return n_rows >= 1 && P >= 1 && C >= 1 && P <= kMaxP && C <= kMaxC && C * P <= kMaxCP;
}
int64_t node_eval_blocks(int64_t n_rows) { return (n_rows + kRows - 1) / kRows; }
int64_t node_eval_sel_blocks(int64_t n_rows, int64_t n_prefix)
{
    return node_eval_blocks(n_prefix < 0 ? 0 : n_prefix < n_rows ? n_prefix : n_rows);
}
size_t node_eval_lds_bytes(int P, int C)
{
    return ((size_t)C * (P | 1) + (size_t)kRows * P + (size_t)kRows * C + 2 * (size_t)kRows + 2) * sizeof(float);
}

}  // namespace

extern "C" size_t sgx_node_eval_workspace_bytes(int64_t n_rows, int64_t n_prefix, int P, int C)
{
    if (!node_eval_shape_ok(n_rows, P, C)) return 0;
    return kHeader + sgx_align_up((size_t)node_eval_sel_blocks(n_rows, n_prefix) * sizeof(BlockRecord), 256);
}

extern "C" int sgx_node_eval(int64_t n_rows, int64_t n_prefix, int P, int C, const float *H, const float *W, const float *bias,
                             const int64_t *target, const uint8_t *mask, int64_t *totals, double *loss_sum, float *logits,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_rows < 1 || n_prefix < 0 || P < 1 || C < 1) return SGX_ERR_SHAPE;
    if (!H || !W || !target || !totals || !loss_sum) return SGX_ERR_NULL;
    if (!node_eval_shape_ok(n_rows, P, C)) return SGX_ERR_UNSUPPORTED;
    const size_t need = sgx_node_eval_workspace_bytes(n_rows, n_prefix, P, C);
    if (!workspace || workspace_bytes < need) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256) return SGX_ERR_ALIGN;
    NodeEvalArgs a;
    a.n_rows = n_rows, a.n_prefix = n_prefix;
    a.n_sel_blocks = node_eval_sel_blocks(n_rows, n_prefix);
    a.n_blocks = logits ? node_eval_blocks(n_rows) : a.n_sel_blocks;       // behind the prefix only the logits want a row
    if (a.n_blocks == 0) return SGX_OK;                      // an empty prefix and no logits wanted: the accumulators stay
    a.P = P, a.C = C, a.pitch_w = P | 1;
    a.H = H, a.W = W, a.bias = bias, a.target = target, a.mask = mask;
    a.totals = totals, a.loss_sum = loss_sum, a.logits = logits;
    a.records = (BlockRecord *)((char *)workspace + kHeader);
    hipStream_t s = (hipStream_t)stream;
    static bool attr_set_on[64] = {};                        // per device (a racing first call sets it twice)
    int dev = 0;
    SGX_HIP_CHECK(hipGetDevice(&dev));
    bool unset = true, &attr_set = dev >= 0 && dev < 64 ? attr_set_on[dev] : unset;
    if (!attr_set) {
        SGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&node_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(((size_t)kMaxCP + kMaxC + (size_t)kRows * kMaxP + (size_t)kRows * kMaxC + 2 * (size_t)kRows + 2) *
                                                sizeof(float))));
        attr_set = true;
    }
    const int grid = (int)(a.n_blocks < kGrid ? a.n_blocks : kGrid);
    hipLaunchKernelGGL(node_eval_kernel, dim3(grid), dim3(kBlock), node_eval_lds_bytes(P, C), s, a);
    SGX_LAUNCH_CHECK();
    if (a.n_sel_blocks == 0) return SGX_OK;                  // logits only
    hipLaunchKernelGGL(node_eval_sum_kernel, dim3(1), dim3(kBlock), 0, s, a);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
