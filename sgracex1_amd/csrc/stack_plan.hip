// The batch plan of the small-graph stack (sgx_batch_plan_*): the checks that graph_ptr cuts a sorted batch into diagonal
// blocks of the adjacency, and the contiguous groups of at most R rows (rows_budget, stack_device.h) that the kernels of
// stack.hip, stack_bwd.hip, stack_gat.hip and stack_quant.hip take one workgroup each.
#include "stack_device.h"

namespace {

constexpr int kTargetGroups = 256;     // one group per CU of an MI355X when the batch is small

struct PlanStatus {
    int bad;          // graph_ptr does not cover [0, n_rows) monotonically, or an edge leaves its graph
    int max_graph;
    int pad[2];
};

__global__ void check_graph_ptr_kernel(int n_rows, int n_graphs, const int32_t *__restrict__ ptr, PlanStatus *st)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_graphs) return;
    const int v = ptr[g];
    if ((g == 0 && v != 0) || (g == n_graphs && v != n_rows)) atomicOr(&st->bad, 1);
    if (g < n_graphs) {
        const int size = ptr[g + 1] - v;
        if (size < 0) atomicOr(&st->bad, 1);
        else atomicMax(&st->max_graph, size);
    }
}

// the graph of row r: the last g with ptr[g] <= r (binary search over ptr[0 .. n_graphs-1])
__device__ __forceinline__ int graph_of(int r, int n_graphs, const int32_t *__restrict__ ptr)
{
    int lo = 0, hi = n_graphs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void check_blocks_kernel(int n_rows, int n_graphs, const int32_t *__restrict__ ptr, const int32_t *__restrict__ rowptr,
                                    const int32_t *__restrict__ col, PlanStatus *st)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int e0 = rowptr[r], e1 = rowptr[r + 1];
    if (e1 < e0) {
        atomicOr(&st->bad, 1);
        return;
    }
    const int g = graph_of(r, n_graphs, ptr);
    const int lo = ptr[g], hi = ptr[g + 1];
    bool ok = true;
    for (int e = e0; e < e1; ++e) {
        const int c = col[e];
        ok = ok && c >= lo && c < hi;
    }
    if (!ok) atomicOr(&st->bad, 1);
}

// group k = the graphs whose first row lies in [k S, (k+1) S); the last group also takes the empty graphs at n_rows
__global__ void group_graphs_kernel(int n_groups, int n_graphs, int S, const int32_t *__restrict__ ptr, int32_t *__restrict__ first)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_groups) return;
    if (k == n_groups) {
        first[k] = n_graphs;
        return;
    }
    const long long start = (long long)k * S;
    int lo = 0, hi = n_graphs;                 // first g with ptr[g] >= start
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)ptr[mid] < start) lo = mid + 1;
        else hi = mid;
    }
    first[k] = k == 0 ? 0 : lo;
}

// S = the window of first rows a group takes: its rows are at most S - 1 + the largest graph <= R; about one group per
// CU for a small batch, full groups for a large one.  Returns the group count of a batch that fits (n_graphs > 0).
int plan_groups(int n_rows, int rows, int max_graph, int *S_out)
{
    const int target = (n_rows + kTargetGroups - 1) / kTargetGroups;
    int S = rows - max_graph + 1;
    if (target < S) S = target;
    if (S < 1) S = 1;
    *S_out = S;
    return n_rows > 0 ? (n_rows + S - 1) / S : 1;
}

// group_graph [n_groups + 1] on the stream; the caller owns (and on an error frees) the table
int launch_group_graphs(int n_groups, int n_graphs, int S, const int32_t *graph_ptr, int32_t *group_graph, hipStream_t s)
{
    hipLaunchKernelGGL(group_graphs_kernel, dim3((unsigned)((n_groups + 1 + 255) / 256)), dim3(256), 0, s, n_groups, n_graphs, S,
                       graph_ptr, group_graph);
    return hipGetLastError() == hipSuccess ? SGX_OK : SGX_ERR_HIP;
}

// what every entry point that takes them asks of these arguments, the shapes first
int check_plan_args(int dtype, int kind, int n_rows, int n_graphs, int max_width)
{
    if (n_rows < 0 || n_graphs < 0 || max_width < 1) return SGX_ERR_SHAPE;
    if (dtype != SGX_F16 && dtype != SGX_F32) return SGX_ERR_UNSUPPORTED;
    if (kind != SGX_BATCH_FORWARD && kind != SGX_BATCH_BACKWARD) return SGX_ERR_UNSUPPORTED;
    return SGX_OK;
}

sgx_batch_plan *make_plan(int dtype, int n_rows, int n_graphs, int max_width, int kind, int max_graph, int fits, int n_groups,
                          int32_t *group_graph, int owns_groups)
{
    return new sgx_batch_plan{dtype, n_rows, n_graphs, max_width, rows_budget(dtype, max_width, kind), n_groups, max_graph, fits,
                              kind, group_graph, owns_groups};                 // (in the order of the struct's fields)
}

}  // namespace

extern "C" int sgx_batch_plan_create_ex(int dtype, int n_rows, int n_graphs, const int32_t *graph_ptr, const int32_t *rowPtr_adj,
                                        const int32_t *columnIndex_adj, int max_width, int kind, sgx_batch_plan **plan,
                                        void *stream)
{
    if (!plan) return SGX_ERR_NULL;
    *plan = nullptr;
    const int rc = check_plan_args(dtype, kind, n_rows, n_graphs, max_width);
    if (rc != SGX_OK) return rc;
    if ((n_rows > 0 || n_graphs > 0) && !graph_ptr) return SGX_ERR_NULL;
    if (n_rows > 0 && (!rowPtr_adj || !columnIndex_adj)) return SGX_ERR_NULL;
    if (n_rows == 0 && n_graphs == 0) {             // nothing to check or to run
        *plan = make_plan(dtype, 0, 0, max_width, kind, 0, 1, 0, nullptr, 1);
        return SGX_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    PlanStatus *st = nullptr;
    auto fail = [&](int status) { if (st) (void)hipFreeAsync(st, s); return status; };
    if (hipMallocAsync((void **)&st, sizeof(PlanStatus), s) != hipSuccess) return fail(SGX_ERR_HIP);
    if (hipMemsetAsync(st, 0, sizeof(PlanStatus), s) != hipSuccess) return fail(SGX_ERR_HIP);
    hipLaunchKernelGGL(check_graph_ptr_kernel, dim3((unsigned)((n_graphs + 1 + 255) / 256)), dim3(256), 0, s, n_rows, n_graphs,
                       graph_ptr, st);
    if (hipGetLastError() != hipSuccess) return fail(SGX_ERR_HIP);
    if (n_rows > 0 && n_graphs > 0) {
        hipLaunchKernelGGL(check_blocks_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, n_rows, n_graphs, graph_ptr,
                           rowPtr_adj, columnIndex_adj, st);
        if (hipGetLastError() != hipSuccess) return fail(SGX_ERR_HIP);
    }
    PlanStatus host;
    if (hipMemcpyAsync(&host, st, sizeof(PlanStatus), hipMemcpyDeviceToHost, s) != hipSuccess) return fail(SGX_ERR_HIP);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(SGX_ERR_HIP);      // the one read-back (16 bytes)
    (void)hipFreeAsync(st, s);
    if (host.bad) return SGX_ERR_BLOCKS;
    const int rows = rows_budget(dtype, max_width, kind);
    const int fits = (rows > 0 && host.max_graph <= rows) ? 1 : 0;
    int n_groups = 0;
    int32_t *group_graph = nullptr;
    if (fits && n_graphs > 0) {
        int S = 1;
        n_groups = plan_groups(n_rows, rows, host.max_graph, &S);
        if (hipMalloc((void **)&group_graph, sizeof(int32_t) * ((size_t)n_groups + 1)) != hipSuccess) return SGX_ERR_HIP;
        if (launch_group_graphs(n_groups, n_graphs, S, graph_ptr, group_graph, s) != SGX_OK) {
            (void)hipFree(group_graph);
            return SGX_ERR_HIP;
        }
    }
    *plan = make_plan(dtype, n_rows, n_graphs, max_width, kind, host.max_graph, fits, n_groups, group_graph, 1);
    return SGX_OK;
}

extern "C" int sgx_batch_plan_create(int dtype, int n_rows, int n_graphs, const int32_t *graph_ptr, const int32_t *rowPtr_adj,
                                     const int32_t *columnIndex_adj, int max_width, sgx_batch_plan **plan, void *stream)
{
    return sgx_batch_plan_create_ex(dtype, n_rows, n_graphs, graph_ptr, rowPtr_adj, columnIndex_adj, max_width,
                                    SGX_BATCH_FORWARD, plan, stream);
}

extern "C" int sgx_batch_plan_destroy(sgx_batch_plan *plan)
{
    if (!plan) return SGX_OK;
    if (plan->group_graph && plan->owns_groups) SGX_HIP_CHECK(hipFree(plan->group_graph));
    delete plan;
    return SGX_OK;
}

extern "C" int sgx_batch_plan_group_count(int dtype, int n_rows, int max_graph, int max_width, int kind)
{
    if (max_graph < 0 || max_graph > n_rows) return SGX_ERR_SHAPE;
    const int rc = check_plan_args(dtype, kind, n_rows, 0, max_width);
    if (rc != SGX_OK) return rc;
    const int rows = rows_budget(dtype, max_width, kind);
    if (rows <= 0 || max_graph > rows) return 0;
    int S = 1;
    return plan_groups(n_rows, rows, max_graph, &S);
}

extern "C" int sgx_batch_plan_create_known(int dtype, int n_rows, int n_graphs, const int32_t *graph_ptr, int max_graph,
                                           int max_width, int kind, int32_t *group_graph, sgx_batch_plan **plan, void *stream)
{
    if (!plan) return SGX_ERR_NULL;
    *plan = nullptr;
    if (max_graph < 0 || max_graph > n_rows) return SGX_ERR_SHAPE;
    if (n_rows > 0 && (n_graphs == 0 || (int64_t)max_graph * n_graphs < n_rows)) return SGX_ERR_SHAPE;
    const int rc = check_plan_args(dtype, kind, n_rows, n_graphs, max_width);
    if (rc != SGX_OK) return rc;
    if ((n_rows > 0 || n_graphs > 0) && !graph_ptr) return SGX_ERR_NULL;
    const int rows = rows_budget(dtype, max_width, kind);
    // the same fields sgx_batch_plan_create_ex records once its checks pass
    const int fits = (n_rows == 0 && n_graphs == 0) ? 1 : ((rows > 0 && max_graph <= rows) ? 1 : 0);
    int S = 1;
    const int n_groups = (fits && n_graphs > 0) ? plan_groups(n_rows, rows, max_graph, &S) : 0;
    if (n_groups > 0 && !group_graph) return SGX_ERR_NULL;
    if (n_groups > 0 && launch_group_graphs(n_groups, n_graphs, S, graph_ptr, group_graph, (hipStream_t)stream) != SGX_OK)
        return SGX_ERR_HIP;
    *plan = make_plan(dtype, n_rows, n_graphs, max_width, kind, max_graph, fits, n_groups, n_groups > 0 ? group_graph : nullptr, 0);
    return SGX_OK;
}

extern "C" int sgx_batch_plan_regroup(const sgx_batch_plan *plan, const int32_t *graph_ptr, void *stream)
{
    if (!plan) return SGX_ERR_NULL;
    if (plan->owns_groups) return SGX_ERR_UNSUPPORTED;      // a checked plan: its table belongs to the batch it was checked on
    if (plan->n_groups == 0) return SGX_OK;                 // no table (the plan does not fit, or has no graph)
    if (!graph_ptr || !plan->group_graph) return SGX_ERR_NULL;
    int S = 1;
    const int n_groups = plan_groups(plan->n_rows, plan->rows, plan->max_graph, &S);      // the S the table was built with
    if (n_groups != plan->n_groups) return SGX_ERR_SHAPE;
    return launch_group_graphs(n_groups, plan->n_graphs, S, graph_ptr, plan->group_graph, (hipStream_t)stream);
}

extern "C" int64_t sgx_batch_plan_export_groups(const sgx_batch_plan *plan, int32_t *dst, int64_t capacity, void *stream)
{
    if (!plan) return SGX_ERR_NULL;
    const int64_t n = plan->group_graph ? (int64_t)plan->n_groups + 1 : 0;
    if (!dst || capacity < n || n == 0) return n;
    SGX_HIP_CHECK(hipMemcpyAsync(dst, plan->group_graph, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return n;
}

extern "C" int sgx_batch_plan_rows(const sgx_batch_plan *plan) { return plan ? plan->rows : SGX_ERR_NULL; }
extern "C" int sgx_batch_plan_groups(const sgx_batch_plan *plan) { return plan ? plan->n_groups : SGX_ERR_NULL; }
extern "C" int sgx_batch_plan_max_graph(const sgx_batch_plan *plan) { return plan ? plan->max_graph : SGX_ERR_NULL; }
extern "C" int sgx_batch_plan_fits(const sgx_batch_plan *plan) { return plan ? plan->fits : SGX_ERR_NULL; }
