// Internal declarations shared by the HIP translation units of libsgx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <atomic>
#include <type_traits>

#include "sgx.h"

#define SGX_HIP_CHECK(expr)                     \
    do {                                        \
        hipError_t _e = (expr);                 \
        if (_e != hipSuccess) return SGX_ERR_HIP; \
    } while (0)

#define SGX_LAUNCH_CHECK()                                   \
    do {                                                     \
        if (hipGetLastError() != hipSuccess) return SGX_ERR_HIP; \
    } while (0)

typedef _Float16 f16;

// A kernel's opt-in to more dynamic LDS than the default (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to that kernel
// ON A DEVICE.  sgx_lds_optin remembers per device that it was made: one object per kernel instantiation, a function-local
// static at the launch site.  sgx_raise_dynamic_lds makes it once per device, before the first launch that needs `bytes`
// or fewer; a device outside the table is opted in on every call (two threads racing on a first call both set it: the
// same value).  SGX_ERR_HIP when the runtime refuses.
struct sgx_lds_optin {
    static constexpr int kDevices = 64;
    std::atomic<bool> done[kDevices];
};
template <typename Kernel>
int sgx_raise_dynamic_lds(Kernel kernel, sgx_lds_optin &optin, size_t bytes)
{
    int dev = 0;
    SGX_HIP_CHECK(hipGetDevice(&dev));
    const bool known = dev >= 0 && dev < sgx_lds_optin::kDevices;
    if (known && optin.done[dev].load(std::memory_order_acquire)) return SGX_OK;
    SGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known) optin.done[dev].store(true, std::memory_order_release);
    return SGX_OK;
}

// Tuning / test overrides: the SGX_* environment variables, read ONCE per process -- not per call: a getenv
// walks the whole environment, and half a dozen of them per layer were a measurable share of a 20-microsecond layer
// (Cora, MUTAG).  Sizing a scratch and launching on it therefore see the same settings.  A process that changes a
// variable afterwards (tests and probes that compare two forms in one process) calls sgx_reload_env().
struct sgx_tuning {
    bool gat_one_pass, gat_no_fused_scores;
    int gat_fused;             // SGX_GAT_FUSED: without E / S outputs the aggregate as one walk (gat_fused.hip): 0 = never, 1 = by shape (default), 2 = wherever it applies
    int gat_scan;              // SGX_GAT_SCAN: 0 = the GAT aggregate's short rows never in entry order, 1 = by shape (default), 2 = always
    bool xw_no_wlds, xw_no_stationary_f32, xw_sparse_no_lds, xw_short_tiles, xw_no_lds;
    bool xtg_scalar, xtg_wave_tiles;
    bool spmm_no_short_tail;      // the one-step tail of a degree order through the sblock path (as in round 2)
    bool layer_no_fused_dense;    // a square dense fp16 layer as two launches (X.W, then A.H) instead of the fused aggregation
    int spmm_fused_blocks_per_cu; // 0 = unset: grid cap of the fused aggregation (workgroups per CU; tools and probes)
    int spmm_cpl;                 // 0 = unset
    int xw_sparse_lpr;            // 0 = unset: lanes per row (slice width / 16 bytes) of the sparse X.W stage's LDS form, at most
    int xw_sparse_streams;        // 0 = unset: streams of row tiles of that form, at most (whole groups of 8; tests and probes)
    int plan_long_threshold;      // 0 = unset
    int plan_chunk;               // 0 = unset
    float plan_reorder_below;     // < 0 = unset
};
const sgx_tuning &sgx_tune();     // util_kernels.hip

static inline size_t sgx_elem_size(int dtype) { return dtype == SGX_F16 ? 2 : 4; }
static inline size_t sgx_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int sgx_next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// The compute units of the current device, for grids sized by them; 256 when the runtime does not say or says fewer than
// `at_least` (what the caller's arithmetic needs: 1, or the 8 of a grid in whole groups of 8).
static inline int sgx_cu_count(int at_least)
{
    int cus = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < at_least)
        cus = 256;
    return cus;
}

// Row schedule (see sgx.h).  Rows with more than `long_threshold` edges are cut into tasks
// of at most `chunk` edges; each task is summed by one wavefront into an fp32 partial row,
// and the partial rows of one long row are added in task order (bitwise reproducible).
struct sgx_plan {
    int n_rows;
    int64_t nnz;
    int long_threshold;
    int chunk;
    int n_long;        // number of long rows
    int n_tasks;       // total edge chunks over all long rows
    // device arrays
    int32_t *long_row;     // [n_long]   row id
    int32_t *long_first;   // [n_long+1] first task of each long row
    int32_t *task_row;     // [n_tasks]
    int32_t *task_e0;      // [n_tasks]
    int32_t *task_e1;      // [n_tasks]
    // Degree-ordered schedule of the rows that are not long (NULL = natural order).  Built only
    // when packing consecutive rows would leave most lane groups idle (power-law graphs): rows are
    // bucketed by the number of 8-edge steps they need, longest first, ascending inside a bucket.
    int32_t *row_order;    // [n_ordered]
    int n_ordered;
    int n_multi;           // the order's rows of two steps and more: row_order[0, n_multi); the rest hold at most 8 edges (-1: no order)
    // The rows of every window of 64 consecutive rows by length, longest first (ties in row order): win_order[64 w + k] =
    // the row (0..63, inside window w) of rank k.  What the LDS form of the sparse X.W stage deals to its sub-tiles
    // (xw_sparse_lds.hip; round 2 sorted every window inside the kernel, 7 % of its instructions); built for the
    // matrices that form can take (2^20 entries and more, no long rows), NULL otherwise.
    uint8_t *win_order;    // [ceil(n_rows / 64) * 64]
    // Where the windows of kScanGranule stored entries meet among the rows, per boundary g = 0 .. n_scan_win (entry
    // g * kScanGranule): scan_win[4 g] = the first row that starts at or behind it, [4 g + 1] = that row's first entry --
    // where the window behind the boundary begins; [4 g + 2], [4 g + 3] = the same pair, or the row before and ITS first
    // entry when that row is a long one (it belongs to the tasks) -- where the window before the boundary ends.  The
    // entry-order form of the GAT aggregate's softmax weights (gat_scan.hip) takes its row-aligned ranges from it; built
    // for plans asked to cut at 256 entries (Csr.gat_plan) that do, or hold no longer row; NULL otherwise.
    int32_t *scan_win;     // [4 (n_scan_win + 1)]
    int64_t n_scan_win;
    float natural_utilization;   // share of lane-group steps doing work when rows are packed in natural order
    int max_degree;              // the longest row (lets a caller skip launches that only serve rows above some length)
};

// leading dimension (elements) the library uses for its own H = X.W scratch.  Rows are padded to a multiple of
// 16 bytes so that every gather is one aligned 16-byte load per lane, and further to whole 128-byte lines where
// that costs at most a third more bytes: a row that straddles a line costs the gather a second line
// (tools/pitch_probe.py, 126 M edges: 47 columns fp16 at pitch 48 / 64: 3.65 / 2.75 ms; 100 columns at pitch
// 104 / 128: 5.58 / 4.59 ms; 72 columns at 72 / 128: 4.51 / 4.57 ms).  Rows under 128 bytes go to the next power
// of two, which never straddles.
static inline int64_t sgx_ldh(int dtype, int P) {
    const int64_t es = dtype == SGX_F16 ? 2 : 4;
    const int64_t row = ((int64_t)P * es + 15) / 16 * 16;
    int64_t pitch = row;
    if (row < 128) {
        pitch = 16;
        while (pitch < row) pitch *= 2;
    } else {
        const int64_t lines = (row + 127) / 128 * 128;
        if (3 * lines <= 4 * row) pitch = lines;
    }
    return pitch / es;
}

// Epilogue of the quantised layer, applied where a stage stores fp32 results (fp16 instantiations ignore it):
//   X.W stage : H = round_decimals(clip(H * rq_shift, +-rq_bound), d) with rq_ten_pow = 10^d   (0 = off; SG.py:607-616)
//   A.H stage : D = act(sum) * out_scale                                                      (0 = off; SG.py:666-667)
// One fp32 operation per rounding point of the reference, as in quant.hip.
struct sgx_epilogue {
    float out_scale, rq_shift, rq_bound, rq_ten_pow;
};
static inline sgx_epilogue sgx_no_epilogue() { return sgx_epilogue{0.0f, 0.0f, 0.0f, 0.0f}; }
sgx_epilogue sgx_requant_epilogue(int scale_fea, int internal_bits);          // quant.hip
// the re-quantisation of one fp32 value of H; contraction must stay off around it
__device__ __forceinline__ float sgx_requant_value(float v, const sgx_epilogue &ep)
{
#pragma clang fp contract(off)
    v = v * ep.rq_shift;
    v = v < -ep.rq_bound ? -ep.rq_bound : v;
    v = v > ep.rq_bound ? ep.rq_bound : v;
    return rintf(v * ep.rq_ten_pow) / ep.rq_ten_pow;
}

// SGX_ACC_REF_HALF stages (refhalf.hip), fp16 only
int sgx_refhalf_csr(int spmm_block, int threads, int relu, int n_rows, int n_cols, int n_feat, const int32_t *rowPtr, const int32_t *columnIndex,
                    const void *values, const void *table, int64_t ldt, void *out, int64_t ldo, hipStream_t s);
int sgx_refhalf_dense(int spmm_block, int threads, int n_rows, int M, int n_feat, const void *X, int64_t ldx, const void *Wt,
                      int64_t ldw, void *out, int64_t ldo, hipStream_t s);

int sgx_spmm_launch(int dtype, int acc_mode, int spmm_block, int relu, int n_rows, int n_cols, int n_feat,
                    const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                    const void *H, int64_t ldh, void *D, int64_t ldd,
                    const sgx_plan *plan, void *scratch, size_t scratch_bytes, hipStream_t stream,
                    const float *acc_in = nullptr, float *acc_out = nullptr, int64_t ld_acc = 0,
                    bool fea_stage = false, int ref_threads = 1, sgx_epilogue ep = sgx_no_epilogue());

// whether a gathered table [n_cols][ldh] is past what 32-bit buffer offsets reach (spmm_csr.hip): 64-bit pointers then
bool sgx_spmm_table_big(int dtype, int n_cols, int64_t ldh, int n_feat);

// The aggregation of a square dense fp16 layer with W applied in its epilogue (spmm_csr.hip): D = act(f16(A.X) . Wt^T) for
// X [n_cols][64], Wt [64][64], D [n_rows][64], all dense -- the bits of sgx_spmm_launch into a Z of pitch 64 followed by
// sgx_xw_dense_ep, without Z in memory.  _applicable: what the kernel asks of the table, the pointers and the plan (the
// layer's own conditions are layer.hip's); the caller checks it first.
bool sgx_spmm_dense_applicable(int n_cols, const void *X, const void *Wt, const void *D, const sgx_plan *plan);
int sgx_spmm_dense(int relu, int n_rows, int n_cols, const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                   const void *X, const void *Wt, void *D, hipStream_t stream);

// X.W for a CSR X with the weight slice resident in LDS (xw_sparse_lds.hip); the caller checks _applicable first
bool sgx_xw_sparse_lds_applicable(int dtype, int n_rows, int m_fea, int n_feat, int64_t ldh, const sgx_plan *plan);
int sgx_xw_sparse_lds(int dtype, int n_rows, int m_fea, int n_feat, const int32_t *rowPtr, const int32_t *columnIndex,
                      const void *values, const void *W, int64_t ldw, void *H, int64_t ldh, const sgx_plan *plan,
                      sgx_epilogue ep, hipStream_t stream);

// sgx_xw_dense / sgx_gat_aggregate with the quantised layer's epilogue (the public entry points pass none)
// rows copied from one pitch to another (util_kernels.hip); dst 16-byte aligned with a pitch that is a multiple of 16
int sgx_repitch_rows(const void *src, int64_t src_pitch, void *dst, int64_t dst_pitch, int row_bytes, int64_t n_rows,
                     hipStream_t stream);
// The arm a dense X.W call takes (what sgx_xw_dense_form packs, include/sgx.h): filled by the function of each file that
// its launch reads too.  kind: SGX_XW_FORM_*; a, b: the template arguments; blocks: column blocks or groups; waves: the
// wavefronts one launch's grid holds (weights-in-LDS: per column block); vec: H stored by vectors.
struct sgx_xw_form {
    int kind, a, b, blocks, vec, wgs_per_cu;
    int64_t waves;
};
// the arm of sgx_xw_dense_wlds / _wlds_f32 for these operands; false = not that kernel's shape
bool sgx_xw_dense_wlds_form(int n_rows, int M, int P, const void *X, int64_t ldx, const void *Wt, int64_t ldw, const void *H,
                            int64_t ldh, sgx_xw_form *form);
bool sgx_xw_dense_wlds_f32_form(int n_rows, int M, int P, const void *Wt, int64_t ldw, const void *H, int64_t ldh, int h_aligned,
                                sgx_xw_form *form);
// X.W, fp16, long K, the weight tile resident in LDS (xw_dense_wlds.hip); SGX_ERR_UNSUPPORTED = not its shape
int sgx_xw_dense_wlds(int n_rows, int M, int P, const void *X, int64_t ldx, const void *Wt, int64_t ldw, void *H, int64_t ldh,
                      int relu, hipStream_t stream);
// the fp32 counterpart for K <= 128 and wide outputs (W^T for all columns in LDS, X read once)
int sgx_xw_dense_wlds_f32(int n_rows, int M, int P, const void *X, int64_t ldx, const void *Wt, int64_t ldw, void *H, int64_t ldh,
                          int h_aligned, sgx_epilogue ep, int relu, hipStream_t stream);
int sgx_xw_dense_ep(int dtype, int acc_mode, int spmm_block, int n_rows, int M_fea, int P, const void *X, int64_t ldx,
                    const void *Wt, int64_t ldw, void *H, int64_t ldh, hipStream_t stream, sgx_epilogue ep, int relu = 0);
int sgx_gat_aggregate_ep(int dtype, int relu, int fill_dead_rows, int n_rows, int n_cols, int n_feat, int n_heads, float alpha,
                         const int32_t *rowPtr, const int32_t *columnIndex, const void *values, const void *Wh, int64_t ldh,
                         const void *attention, void *D, int64_t ldd, float *E, float *S, const sgx_plan *plan,
                         float *s_scratch, hipStream_t stream, float out_scale, const float *ext_fill = nullptr, int ext_n = 0,
                         int scores_ready = 0);

// The GAT aggregate's one scratch buffer (sgx_gat_scratch_bytes floats behind s_scratch), laid out in ONE place
// (sgx_gat_scratch_layout, gat.hip): the float offset of every region.  A region the call does not have is empty and
// carries the offset of what follows it.
struct sgx_gat_scratch {
    size_t s1, s2;                        // the scores Wh.a1 / Wh.a2, [n_cols][n_heads] each
    size_t slabs, mean;                   // fill_dead_rows: the column-sum slabs [slabs][n_feat], then the mean row [n_feat]
    size_t sp1, sp2;                      // has_partials: the X.W epilogue's score partials, [n_cols][n_feat / 64] each
    size_t pacc, pm, pl;                  // has_split: per task of the plan an fp32 partial row [ldp], (max, sum) per head
    size_t row_m, row_l;                  //            per long row (max, sum) per head
    size_t weights, dead;                 // has_two_stage: stage A's weights [nnz][n_heads], then the dead-row flags ([n_rows] bytes)
    size_t total;                         // floats in all
    int ldp;                              // pitch of a partial row
    bool has_partials, has_split, has_two_stage;
};
sgx_gat_scratch sgx_gat_scratch_layout(int n_cols, int n_feat, int n_heads, int fill_dead_rows, const sgx_plan *plan);

// One call of the aggregate, as its forms see it (gat.hip fills it in and chooses the form)
struct sgx_gat_args {
    int dtype, lpr;            // element type and lanes per row: with vec_ok the kernels' template arguments (sgx_gat_dispatch)
    int relu, n_rows, n_cols, n_feat, n_heads;
    float alpha;
    const int32_t *rowptr, *col;
    const void *val, *Wh, *att;
    int64_t ldh, ldd;
    unsigned h_bytes, ld_bytes;
    void *D;
    float *E, *S;
    float *scratch;            // the caller's scratch
    sgx_gat_scratch lay;       // and where everything lies in it
    const float *fill;
    int uniform_n;             // the N of the uniform softmax a dead row gets (S = 1/N): n_cols, or all nodes of a partitioned graph
    float out_scale;           // deq_o of the quantised layer on fp32 outputs (0 = off)
    const sgx_plan *plan_any;  // the caller's plan, long rows or not (two-stage form: it tells the stored-entry count)
    const sgx_plan *plan;      // long rows -> split path
    int vec_ok, vec_store;
    int scores_ready;          // the scratch already holds Wh.a1 / Wh.a2 (formed in the epilogue of the X.W kernel that produced Wh)
    hipStream_t stream;
};

// The kernels' template arguments from a call's runtime facts, for every form: f(T(), VEC, LPR) with the element type, the
// elements a lane holds (16 bytes where the table allows, else 1) and the lanes per row as integral constants.
template <typename T, int VEC, typename F>
int sgx_gat_dispatch_lpr(int lpr, F &&f)
{
    switch (lpr) {
    case 1: return f(T(), std::integral_constant<int, VEC>(), std::integral_constant<int, 1>());
    case 2: return f(T(), std::integral_constant<int, VEC>(), std::integral_constant<int, 2>());
    case 4: return f(T(), std::integral_constant<int, VEC>(), std::integral_constant<int, 4>());
    case 8: return f(T(), std::integral_constant<int, VEC>(), std::integral_constant<int, 8>());
    case 16: return f(T(), std::integral_constant<int, VEC>(), std::integral_constant<int, 16>());
    case 32: return f(T(), std::integral_constant<int, VEC>(), std::integral_constant<int, 32>());
    default: return f(T(), std::integral_constant<int, VEC>(), std::integral_constant<int, 64>());
    }
}
template <typename F>
int sgx_gat_dispatch(const sgx_gat_args &a, F &&f)
{
    if (a.dtype == SGX_F16) return a.vec_ok ? sgx_gat_dispatch_lpr<f16, 8>(a.lpr, f) : sgx_gat_dispatch_lpr<f16, 1>(a.lpr, f);
    return a.vec_ok ? sgx_gat_dispatch_lpr<float, 4>(a.lpr, f) : sgx_gat_dispatch_lpr<float, 1>(a.lpr, f);
}
// The element type alone: f(T()) with f16 for SGX_F16 and float otherwise, so that the launch of kernel<T> is written once.
template <typename F>
int sgx_dtype_dispatch(int dtype, F &&f)
{
    return dtype == SGX_F16 ? f(f16()) : f(float());
}

// gat.hip, for the forms and for sgx_gat_aggregate_flat (gat_flat.hip), which lays out a scratch of its own: the lane split
// of a call (vec_ok, vec_store, lpr), its score pre-pass into a.scratch at a.lay.s1 / s2, and the mean row of Wh that the
// dead rows of fill_dead_rows receive (slabs: sgx_gat_mean_slab_floats(n_feat) floats)
void sgx_gat_lane_split(sgx_gat_args &a);
int sgx_gat_scores_launch(const sgx_gat_args &a);
size_t sgx_gat_mean_slab_floats(int n_feat);
int sgx_gat_mean_row(int dtype, int n_cols, int n_feat, const void *Wh, int64_t ldh, float *slabs, float *mean, hipStream_t stream);

// The forms of the aggregate behind gat.hip's choice, each on scores already in the scratch:
// gat_one_pass.hip: one walk per row with a running softmax state (any adjacency, no plan needed; E / S optional)
int sgx_gat_one_pass(const sgx_gat_args &a);
// gat_alpha.hip: stage A of the two-stage form by rows -- the softmax weights of the stored entries into W (the caller's S
// or the scratch), the dead-row flags, E; scan: the rows up to the plan's cut in entry order instead (gat_scan.hip)
int sgx_gat_alpha_stage(const sgx_gat_args &a, float *W, bool scan);
// gat_weighted.hip: stage B -- D = act(sum_e W_e Wh[col_e]) and the dead rows' fill
int sgx_gat_weighted(const sgx_gat_args &a, const float *W);
// gat_stats.hip: the row softmax statistics (sgx_gat_stats) of an aggregate that has just run on s_scratch, from the scores
// its pre-pass left there; sgx_gat_stats_check: SGX_ERR_NULL for a missing array, SGX_ERR_UNSUPPORTED past 32-bit offsets
int sgx_gat_stats_check(const sgx_gat_stats *st, int n_cols, int n_heads);
int sgx_gat_row_stats(int dtype, int n_rows, int n_cols, int n_heads, float alpha, const int32_t *rowPtr,
                      const int32_t *columnIndex, const void *values, const float *s_scratch, const sgx_gat_scratch &lay,
                      const sgx_gat_stats *st, hipStream_t stream);
// gat_scan.hip: the softmax weights of the stored entries of every row of up to kScanMaxRow entries (stage A of the
// two-stage aggregate) as a segmented scan in entry order; longer rows are the plan's tasks
constexpr int kScanGranule = 64, kScanMaxRow = 256;
bool sgx_gat_scan_applicable(const sgx_plan *plan);
int sgx_gat_alpha_scan(int dtype, int n_rows, int n_heads, const sgx_plan *plan, const int32_t *rowptr, const int32_t *col,
                       const void *val, const float *s1, const float *s2, float alpha, float *W, float *E, unsigned char *dead,
                       hipStream_t stream);

// gat_fused.hip: the GAT aggregate in one walk, the neighbours' scores formed from the rows it gathers (no E / S outputs)
struct sgx_gat_fused_args {
    int dtype, lpr, relu, n_rows, n_feat, n_heads, vec_store, ldp;
    float alpha, out_scale;
    const sgx_plan *plan;      // its row schedule (row_schedule.h)
    const int32_t *rowptr, *col;
    const void *val, *Wh, *att;
    unsigned h_bytes, ld_bytes;
    const float *s1, *fill;
    void *D;
    int64_t ldd;
    float *pacc, *pm, *pl;
    hipStream_t stream;
};
bool sgx_gat_fused_applicable(int dtype, int n_feat, int n_heads, int lpr);
int sgx_gat_fused(const sgx_gat_fused_args &a);

// GAT layer: the attention scores formed by the X.W kernel's epilogue (fp16, heads of 32 columns, two-stage aggregate)
bool sgx_gat_scores_fusable(int dtype, int n_feat, int n_heads, const sgx_plan *plan);
int sgx_gat_scores_combine(float *s_scratch, const sgx_gat_scratch &lay, int n_cols, int n_feat, int n_heads, hipStream_t stream);
// sgx_xw_dense_ep for that case: s1 / s2 [n_rows x n_heads] = H.a1 / H.a2 per head beside H; SGX_ERR_UNSUPPORTED when
// the shape is not the stationary kernel's (the caller then runs the plain product and lets the aggregate form the scores)
// (heads of 32 columns: s1 / s2 are the scores themselves; heads of 64 columns and more: one partial per (row, 64-column
// group), [n_rows x P / 64] each, for sgx_gat_scores_combine)
int sgx_xw_dense_scores(int n_rows, int M_fea, int P, const void *X, int64_t ldx, const void *Wt, int64_t ldw, void *H, int64_t ldh,
                        const void *attention, int n_heads, float *s1, float *s2, hipStream_t stream);
