// The classifier tail of an evaluation pass over node batches in one call (sgx_node_eval, include/sgx.h "the node
// evaluation head"): the C x P Linear head on the SELECTED rows of a node matrix (a prefix, a byte mask, or both), the
// per-row cross entropy and the arg-max's hit, ADDED to accumulators that stay on the device across the batches of a pass
// -- totals[0] += selected rows, totals[1] += hits, loss_sum += the summed loss.  What demo_sgrace.py's test(loader, split)
// runs per batch as model(...), out[:batch_size], argmax, ==, sum and a read-back.
//
// Two launches, as sgx_head_eval.  In the first a workgroup takes the row blocks b, b + grid, ... of SGX_NODE_LOSS_ROWS
// rows, each up to its logits by tail_device.h's node_block_front without dropout -- sgx_node_loss's front, so the logits
// are its logits at p = 0; a thread per selected row forms lse, the loss and the arg-max (row_cross_entropy), and thread 0
// adds the block's selected rows' losses in row order into a double and stores the block's record -- that double, the rows
// it selected, its hits -- in the block's own workspace slot.  Nothing that is summed depends on the grid.  The second, one
// workgroup: the records' integers, then their doubles added in block order (ordered_sum), and all three added to the
// accumulators.  No atomics: the same bits on every run and for any grid.
#include "tail_device.h"

using namespace sgx_tail;

namespace {

constexpr size_t kHeader = 256;                             // the workspace's first 256 bytes are reserved

struct BlockRecord {                  // one per block of kRows rows that can hold a selected row
    double loss;                      // its selected rows' fp32 losses, added from 0.0 in row order
    int32_t rows, hits;
};
static_assert(sizeof(BlockRecord) == 16, "the workspace rule counts 16 bytes a block");

struct NodeEvalArgs {
    NodeRows r;
    int64_t n_blocks, n_sel_blocks;   // blocks the first launch walks; blocks that own a record
    const int64_t *target;
    int64_t *totals;
    double *loss_sum;
    BlockRecord *records;             // [n_sel_blocks]
};

__global__ __launch_bounds__(kBlock) void node_eval_kernel(NodeEvalArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char node_eval_lds[];
    const int tid = threadIdx.x;
    const int P = a.r.P, C = a.r.C;
    float *const Ws = reinterpret_cast<float *>(node_eval_lds);   // [C][pitch]; the layout is node_eval_lds_bytes's
    float *const xs = Ws + (size_t)C * a.r.pitch_w;               // [kRows][P]
    float *const zs = xs + (size_t)kRows * P;                     // [kRows][C]
    float *const loss_s = zs + (size_t)kRows * C;                 // [kRows]
    int *const hit_s = reinterpret_cast<int *>(loss_s + kRows);   // [kRows]
    unsigned *const sel_s = reinterpret_cast<unsigned *>(hit_s + kRows);   // [2], by the parity of the iteration
    bool w_ready = false;
    int it = 0;
    for (int64_t b = blockIdx.x; b < a.n_blocks; b += gridDim.x, it ^= 1) {
        const NodeBlock blk = node_block_front<false>(a.r, b, it, w_ready, Ws, xs, zs, sel_s);
        const unsigned selbits = blk.selbits;
        if (blk.needbits == 0) {                            // nothing to compute: H is not read
            if (tid == 0 && b < a.n_sel_blocks) a.records[b] = BlockRecord{0.0, 0, 0};
            continue;
        }
        if (tid < kRows) {
            float loss = 0.0f;
            int hit = 0;
            if ((selbits >> tid) & 1u) {
                const float *z = zs + tid * C;
                const int64_t t = a.target[blk.base + tid];
                const RowCe ce = row_cross_entropy(z, C, t);
                if (ce.live) {
                    loss = ce.lse - z[t];
                    hit = ce.best == (int)t;
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
    const double sum = ordered_sum(a.n_sel_blocks, chunk, [&](int64_t k) { return a.records[k].loss; });      // thread 0's
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

int64_t node_eval_sel_blocks(int64_t n_rows, int64_t n_prefix)
{
    return row_blocks(n_prefix < 0 ? 0 : n_prefix < n_rows ? n_prefix : n_rows);
}

}  // namespace

extern "C" size_t sgx_node_eval_workspace_bytes(int64_t n_rows, int64_t n_prefix, int P, int C)
{
    if (!node_shape_ok(n_rows, P, C)) return 0;
    return kHeader + sgx_align_up((size_t)node_eval_sel_blocks(n_rows, n_prefix) * sizeof(BlockRecord), 256);
}

extern "C" int sgx_node_eval(int64_t n_rows, int64_t n_prefix, int P, int C, const float *H, const float *W, const float *bias,
                             const int64_t *target, const uint8_t *mask, int64_t *totals, double *loss_sum, float *logits,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_rows < 1 || n_prefix < 0 || P < 1 || C < 1) return SGX_ERR_SHAPE;
    if (!H || !W || !target || !totals || !loss_sum) return SGX_ERR_NULL;
    if (!node_shape_ok(n_rows, P, C)) return SGX_ERR_UNSUPPORTED;
    const size_t need = sgx_node_eval_workspace_bytes(n_rows, n_prefix, P, C);
    if (!workspace || workspace_bytes < need) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256) return SGX_ERR_ALIGN;
    NodeEvalArgs a;
    a.r = NodeRows{n_rows, n_prefix, P, C, P | 1, H, W, bias, mask, logits};
    a.n_sel_blocks = node_eval_sel_blocks(n_rows, n_prefix);
    a.n_blocks = logits ? row_blocks(n_rows) : a.n_sel_blocks;             // behind the prefix only the logits want a row
    if (a.n_blocks == 0) return SGX_OK;                      // an empty prefix and no logits wanted: the accumulators stay
    a.target = target, a.totals = totals, a.loss_sum = loss_sum;
    a.records = (BlockRecord *)((char *)workspace + kHeader);
    hipStream_t s = (hipStream_t)stream;
    static sgx_lds_optin optin;
    const int rc = sgx_raise_dynamic_lds(&node_eval_kernel, optin, kNodeEvalLdsMax);
    if (rc != SGX_OK) return rc;
    const int grid = (int)(a.n_blocks < kGrid ? a.n_blocks : kGrid);
    hipLaunchKernelGGL(node_eval_kernel, dim3(grid), dim3(kBlock), node_eval_lds_bytes(P, C), s, a);
    SGX_LAUNCH_CHECK();
    if (a.n_sel_blocks == 0) return SGX_OK;                  // logits only
    hipLaunchKernelGGL(node_eval_sum_kernel, dim3(1), dim3(kBlock), 0, s, a);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
