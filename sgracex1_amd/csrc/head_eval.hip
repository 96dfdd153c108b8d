// The classifier tail of an evaluation pass in one call (sgx_head_eval, include/sgx.h "the evaluation head"): the C x P
// Linear head on the pooled means, the per-graph cross entropy and the arg-max's hit, ADDED to accumulators that stay on
// the device across the batches of a pass -- totals[0] += real graphs, totals[1] += hits, loss_sum += the summed loss.
// What the notebook's accuracy() runs as self.lin, argmax, ==, sum and a read-back per set.
//
// Two launches, as sgx_head_loss.  The first, a wavefront per graph: wave w of workgroup b takes the graphs 4 b + w,
// 4 b + w + 4 grid, ...; per graph the logits (tail_device.h: wave_class_logit, on pooled itself: p_drop = 0), then
// lane 0 forms lse, the loss and the arg-max (row_cross_entropy), stores the graph's fp32 loss in its own workspace slot
// and counts its hits.  Nothing that is summed depends on the grid: the loss slots are per graph, the hit counts are
// integers.  The second, one workgroup: the slots added in graph order into a double (ordered_sum), the counts, and both
// added to the accumulators.  No atomics: the same bits on every run and for any grid.
// (A one-launch form -- the last workgroup to draw a ticket, zeroed by a memset node, doing the second launch's work behind
// an agent-scope release / acquire -- passed every test and then lost whole calls' sums after some tens of back-to-back
// graph replays (tools/eval_probe.py: a pass counted 0 graphs); the cause was not established, and the launch boundary
// it saved is about 2 us.)
#include "tail_device.h"

using namespace sgx_tail;

namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kEvalGrid = 256;        // workgroups at most
constexpr size_t kHeader = 256;       // the workspace's first 256 bytes are reserved

struct EvalArgs {
    int G, n_real, P, C;
    const float *pooled, *W, *bias;
    const int64_t *target;
    int64_t *totals;
    double *loss_sum;
    float *logits;
    float *row_loss;                  // [G]: graph g's loss, rows below n_real only
    int *wave_hits;                   // [grid * kWaves]
};

__global__ __launch_bounds__(kBlock) void head_eval_kernel(EvalArgs a)
{
#pragma clang fp contract(off)
    __shared__ float zs[kWaves][kMaxC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = a.P, C = a.C;
    const int rows = a.logits ? a.G : a.n_real;              // the filler graphs are read for the logits output only
    const int n_waves = (int)gridDim.x * kWaves;
    float *z = zs[wave];
    int hits = 0;                                            // lane 0's
    for (int g = (int)blockIdx.x * kWaves + wave; g < rows; g += n_waves) {
        const float *xs = a.pooled + (int64_t)g * P;         // p_drop = 0: x == pooled bit for bit
        for (int c = 0; c < C; ++c) {
            const float s = wave_class_logit(a.W + (int64_t)c * P, xs, P, lane, a.bias, c);
            if (lane == 0) {
                z[c] = s;
                if (a.logits) a.logits[(int64_t)g * C + c] = s;
            }
        }
        if (lane == 0 && g < a.n_real) {                     // z is lane 0's own: written and read by the one thread
            const int64_t t = a.target[g];
            const RowCe ce = row_cross_entropy(z, C, t);
            a.row_loss[g] = ce.live ? ce.lse - z[t] : 0.0f;
            hits += ce.live && ce.best == (int)t;
        }
    }
    if (lane == 0) a.wave_hits[(int)blockIdx.x * kWaves + wave] = hits;
}

// the sums, by one workgroup: the hit counts (integers, any order), then the loss slots in graph order, fed through LDS
__global__ __launch_bounds__(kBlock) void head_eval_sum_kernel(EvalArgs a, int n_waves)
{
    __shared__ float chunk[kBlock];
    __shared__ int hits_s[kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int h = 0;
    for (int k = tid; k < n_waves; k += kBlock) h += a.wave_hits[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
    if (lane == 0) hits_s[wave] = h;
    const double sum = ordered_sum(a.n_real, chunk, [&](int k) { return a.row_loss[k]; });      // thread 0's
    __syncthreads();
    if (tid == 0) {
        int64_t n = 0;
        for (int w = 0; w < kWaves; ++w) n += hits_s[w];
        a.totals[0] += a.n_real;
        a.totals[1] += n;
        a.loss_sum[0] += sum;
    }
}

}  // namespace

extern "C" size_t sgx_head_eval_workspace_bytes(int n_graphs, int P, int C)
{
    if (!head_shape_ok(n_graphs, P, C)) return 0;
    return kHeader + sgx_align_up((size_t)n_graphs * sizeof(float), 256) + (size_t)kEvalGrid * kWaves * sizeof(int);
}

extern "C" int sgx_head_eval(int n_graphs, int n_real, int P, int C, const float *pooled, const float *W, const float *bias,
                             const int64_t *target, int64_t *totals, double *loss_sum, float *logits, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    if (n_graphs < 1 || n_real < 0 || n_real > n_graphs || P < 1 || C < 1) return SGX_ERR_SHAPE;
    if (!pooled || !W || !target || !totals || !loss_sum) return SGX_ERR_NULL;
    if (P > kMaxP || C > kMaxC) return SGX_ERR_UNSUPPORTED;
    const size_t need = sgx_head_eval_workspace_bytes(n_graphs, P, C);
    if (!workspace || workspace_bytes < need) return SGX_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256) return SGX_ERR_ALIGN;
    const int rows = logits ? n_graphs : n_real;
    if (rows == 0) return SGX_OK;                            // no real graph and no logits wanted: the accumulators stay
    EvalArgs a;
    a.G = n_graphs, a.n_real = n_real, a.P = P, a.C = C;
    a.pooled = pooled, a.W = W, a.bias = bias, a.target = target;
    a.totals = totals, a.loss_sum = loss_sum, a.logits = logits;
    a.row_loss = (float *)((char *)workspace + kHeader);
    a.wave_hits = (int *)((char *)workspace + kHeader + sgx_align_up((size_t)n_graphs * sizeof(float), 256));
    const int blocks = (rows + kWaves - 1) / kWaves;
    const int grid = blocks < kEvalGrid ? blocks : kEvalGrid;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(head_eval_kernel, dim3(grid), dim3(kBlock), 0, s, a);
    SGX_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_eval_sum_kernel, dim3(1), dim3(kBlock), 0, s, a, grid * kWaves);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
