/*
 * sgx.h -- C ABI of libsgx.so, the MI355X (gfx950) replacement for the one device
 * kernel of hadimsnj/SGRACEx1: the fused GNN layer  D = act( A . (X . W) ).
 *
 * Every entry point below is what the reference's host code binds for this path.
 * Citations are relative to the reference checkout:
 *   K.cpp  = gnn-rfsoc-mt-all-2022/src/kernelMatrixmult_all.cpp
 *   KH     = gnn-rfsoc-mt-all-2022/src/kernelMatrixmult.h
 *   MM.h   = gnn-rfsoc-mt-all-2022/src/matrix_mult.h
 *   MOL    = jupyter/molecule_gcn/Graph_Classification.ipynb   (cell numbers, 0-based)
 *   MMN    = jupyter/test/mmult-master.ipynb
 *   SG.py  = demo/sgrace_lib/sgrace.py
 *
 * Conventions (same as the reference, K.cpp:3762-3774):
 *   - all matrix pointers are DEVICE pointers (HBM), caller-owned; the library only
 *     reads inputs and writes D / E / S / the workspace;
 *   - indices are int32, zero based; CSR = rowPtr[N+1], columnIndex[nnz], values[nnz]; the number of
 *     stored entries is read from rowPtr on the device, so columnIndex / values must be valid
 *     pointers even for a matrix without entries (nothing is read through them then);
 *   - B holds the weights TRANSPOSED, [P_w][M_fea] row-major (K.cpp:3043, MOL cell 16);
 *   - D is [N_adj][P_w] row-major; the feature matrix has M_adj rows (K.cpp:3734);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous on that stream and re-entrant per stream; they never synchronise,
 *     allocate or free, so they can be captured in a hipGraph;
 *   - return value: SGX_OK (0) or a negative sgx_status.  The reference validates
 *     nothing and returns nothing (K.cpp:3762); the argument checks are new.
 */
#ifndef SGX_H
#define SGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGX_VERSION 110

typedef enum sgx_status {
    SGX_OK = 0,
    SGX_ERR_NULL = -1,         /* a required pointer is NULL                         */
    SGX_ERR_SHAPE = -2,        /* a dimension is negative / zero where it may not be */
    SGX_ERR_UNSUPPORTED = -3,  /* dtype / mode not built                             */
    SGX_ERR_WORKSPACE = -4,    /* workspace missing or too small                     */
    SGX_ERR_HIP = -5,          /* a HIP call or launch failed                        */
    SGX_ERR_CSR = -6,          /* sgx_csr_validate: rowPtr not monotone / index out of range */
    SGX_ERR_ALIGN = -7,        /* pointer or leading dimension not aligned as required */
    SGX_ERR_SEEDS = -8,        /* sgx_sample_neighbors: a seed repeats or lies outside [0, n_nodes) */
    SGX_ERR_BLOCKS = -9        /* sgx_batch_plan_create: graph_ptr does not cut the adjacency into diagonal blocks */
} sgx_status;

/* Element type of B, D, values_fea, values_adj (MM.h:76-148 selects ONE type for all:
 * HALF in the live build, FLOAT optional; SG.py:1545 allocates float32 buffers). */
typedef enum sgx_dtype { SGX_F16 = 0, SGX_F32 = 1 } sgx_dtype;

/* How sums are formed.
 *   SGX_ACC_F32       products and sums in fp32, one rounding to the storage type at the
 *                     end (default; compared with the exact oracle at a stated tolerance).
 *   SGX_ACC_REF_HALF  fp16 only: every product and every add rounded to binary16, element
 *                     k of an sblock accumulated in partial-sum lane k mod 4, lanes folded
 *                     ((p0+p1)+p2)+p3 -- the arithmetic of the reference's HALF build
 *                     (K.cpp:1829-1884, :2009-2061; MM.h:137-138), bit for bit.       */
typedef enum sgx_acc_mode { SGX_ACC_F32 = 0, SGX_ACC_REF_HALF = 1 } sgx_acc_mode;

/* ---- row schedule of a CSR matrix ------------------------------------------------
 * The reference splits rows over ADJ_THREADS / FEA_THREADS by row count and groups
 * SPMM_BLOCK rows per pipelined loop (K.cpp:3517-3523, :826-845; MM.h:166-191).  On the
 * GPU the same two decisions are made once per matrix: which rows are packed several to
 * a wavefront (the sblock path) and which are long enough to be cut into edge chunks
 * handled by separate wavefronts.  A plan is optional: without one every row takes the
 * sblock path (correct, slower on power-law graphs). */
typedef struct sgx_plan sgx_plan;

/* Builds the plan for rowPtr (device), on the device (csrc/plan_build.hip): the host reads back the entry count and
 * then the number of long rows / tasks it has to size arrays for -- 28 bytes, never rowPtr -- so `stream` is
 * synchronised twice (the fill kernels are still in flight on `stream` when this returns; the builder's scratch comes
 * from the stream-ordered pool); not capturable.
 * n_feat_hint is unused (kept for callers of the first version). */
int sgx_plan_create(sgx_plan **plan, const int32_t *rowPtr, int n_rows, int n_feat_hint,
                    void *stream);
/* The same with the cut chosen by the caller: rows over `long_threshold` edges are split into tasks of `chunk`
 * edges (0 = the default: both sqrt(nnz) / 2 rounded down to a power of two, 64 .. 4096 -- the measured optimum of the A.H
 * aggregation moves with the size of the graph; the first stage of the GAT aggregate runs best with 256 / 256).
 * Matrices under 2^20 entries always use 64 / 64; a cut above 65536 is taken as 65536. */
int sgx_plan_create_ex(sgx_plan **plan, const int32_t *rowPtr, int n_rows, int long_threshold, int chunk,
                       void *stream);
void sgx_plan_destroy(sgx_plan *plan);
/* number of rows that take the split path, and the edge count above which a row does (for reports /
 * tests): sqrt(nnz) / 2 as a power of two (at most 4096) by default, 64 for matrices under 2^20 stored entries, whose
 * run time is the longest row's chain of dependent steps */
int sgx_plan_long_rows(const sgx_plan *plan);
int sgx_plan_long_threshold(const sgx_plan *plan);
/* share of lane-group steps that do work when 8 consecutive rows are packed per wavefront, and
 * whether the plan therefore schedules the short rows in degree order instead (1) or not (0) */
float sgx_plan_natural_utilization(const sgx_plan *plan);
int sgx_plan_reordered(const sgx_plan *plan);
/* One of the plan's device arrays copied to dst (device, int32, `capacity` entries) for inspection and tests:
 * which = 0 long_row, 1 long_first, 2 task_row, 3 task_e0, 4 task_e1, 5 row_order, 6 win_order (the rows of every 64-row
 * window by length, one byte per row, four to an int32; built for matrices of 2^20 entries and more without long rows),
 * 7 scan_win (per boundary g = 0 .. ceil(nnz / 64) between windows of 64 stored entries: the first row starting at or
 * behind entry 64 g and its first entry, then the same pair or -- when the row before is a long one -- that row and its
 * first entry: the row-aligned entry ranges of the GAT aggregate's scan; built for plans created with a cut of 256 entries that are cut there or hold no
 * longer row).  Returns the array's length
 * (dst NULL: the length only) or a negative sgx error. */
int64_t sgx_plan_export(const sgx_plan *plan, int which, int32_t *dst, int64_t capacity, void *stream);
/* Which kernel form sgx_xw_sparse (and the first stage of sgx_layer_forward in gemm_mode 0) takes for these operands, for
 * reports and tests (added without a version bump, SGX_VERSION stays 110: a new declaration, nothing else changes): a
 * host query without a launch, answered by the functions the launch itself uses.  0 = the gather
 * kernel (W read through L2); otherwise the form with W's column slices resident in LDS, as
 *   lpr | n_split << 8 | full << 16 | w_vec << 17 | wgs_per_cu << 18 | streams << 20
 * lpr = lanes per row (2, 4, 8, 16; a slice is lpr x 16 bytes wide), n_split = column slices (1 .. 4), full = one 16-byte
 * store per lane and row (P a multiple of the slice width, H and its pitch 16-byte aligned; element stores otherwise),
 * w_vec = the slice filled with 16-byte loads (W and its pitch 16-byte aligned), wgs_per_cu = workgroups a CU holds
 * (1, 2), streams = the row-tile streams of the persistent grid (a multiple of 8; window w of 64 rows belongs to
 * wavefront w mod 16 streams).  W, H: the pointers the call would get (only their alignment is read); ldw, ldh in elements. */
int sgx_xw_sparse_form(int dtype, int n_rows, int M_fea, int P, const void *W, int64_t ldw, const void *H, int64_t ldh,
                       const sgx_plan *plan);

/* ---- quantised layer of the SGRACE bitstream (SG.py:53-265, :570-667, :1645-1848) -------
 * The reference quantises inside the device kernel from scale registers and states the arithmetic
 * in its emulation branch (SG.py:570-667): features and adjacency values go to an unsigned w_qbits
 * grid, weights and the attention vector to a signed one, each put back on a fractional grid
 * (x_q / 2^(w_qbits-1)); H = X.W is divided by 2^scale_fea, clipped to +-(2^ib - 1)/2^ib and rounded
 * to ib - 1 decimals (ib = internal_quantization); after aggregation and ReLU the result is
 * multiplied by deq_o.  All of it in fp32 (dtype must be SGX_F32).  The fields are the registers of
 * the GAT bitstream (SG.py:335-365, :476; demo/zcu104/gat_all_unsigned.hwh). */
#define SGX_QUANT_ADJ_DONE 1   /* flags: values_adj already hold quantised values (graph cached by the host) */
#define SGX_QUANT_INT8 2       /* flags: gemm_mode 1, qbits <= 8, P_w <= 256: X and W go to the int8 matrix cores as the
                                  integer codes of their grids (sgx_quantize_codes_i8 + sgx_xw_dense_i8) -- X.W summed
                                  exactly in int32 instead of in fp32, X read as 1 byte per element.  Equal to the fp32
                                  form whenever that form's sums are exact (|sum of code products| < 2^24), to fp32
                                  rounding otherwise.  Ignored (fp32 form) where it does not apply.              */
#define SGX_QUANT_INT8_AUTO 4  /* flags: the integer operands where they are the faster form -- M_fea > 128, i.e. where
                                  the fp32 product no longer has its weights-stationary kernels (those hold W for
                                  K <= 128: at K = 128 the two forms tie, at Reddit's 602 the integer form takes half
                                  the time, X being read as bytes).  What `config.hardware_quantize = 1` selects in
                                  the SGRACE library's layers (SG.py:570-616: the bitstream's own quantiser).       */
#define SGX_QUANT_FLAT 8       /* flags: the opt-in of the quantised layer to SGX_SCHEDULE_FLAT ("quantised layer on the
                                  entry-split schedule" under sgx_layer_desc.schedule_adj).  Without it a descriptor
                                  with `quant` and SGX_SCHEDULE_FLAT is refused as before; read nowhere else.        */
typedef struct sgx_quant {
    int32_t qbits;              /* config.w_qbits: 8, 4, 2 or 1                                       */
    int32_t scale_fea;          /* register scale_fea                                                 */
    int32_t internal_bits;      /* register quantized_multiplier = internal_quantization (SG.py:476)  */
    int32_t flags;
    float   inv_scale_fea;      /* register quantization_scale_fea = 1 / f_s                          */
    float   zero_fea;           /* f_z                                                                */
    float   inv_scale_w;        /* register quantization_scale_w = 1 / w_s (also used for `attention`) */
    float   zero_w;             /* w_z                                                                */
    float   inv_scale_adj;      /* register quantization_scale_adj = 1 / a_s                          */
    float   zero_adj;           /* a_z                                                                */
    float   deq_factor;         /* register deq_factor = deq_o                                        */
    float   reserved;
    int64_t nnz_adj;            /* registers nnz_adj1..4 (SG.py:1205-1260): stored entries of A       */
    int64_t nnz_fea;            /* registers nnz_fea1..4: stored entries of X (gemm_mode 0)           */
} sgx_quant;

/* The two rounding steps on their own (fp32, device pointers; out may alias x):
 *   out = clip(round(inv_scale * x + zero), lo, hi) / 2^(qbits-1)   unsigned: lo = 0, hi = 2^qbits - 1
 *                                                                   signed:   -+(2^(qbits-1) - 1)
 *   qbits = 1: signed -> -0.5 / +0.5 by sign (SG.py:177-182), unsigned -> clip(round, 0, 1) / 2 (SG.py:184-189)
 *   H = round_decimals(clip(H / 2^scale_fea, +-(2^ib - 1) / 2^ib), ib - 1), in place (SG.py:607-616) */
int sgx_fake_quantize(int is_signed, int qbits, float inv_scale, float zero, int64_t n, const float *x,
                      float *out, void *stream);
int sgx_requantize(int n_rows, int n_feat, int64_t ld, float *H, int scale_fea, int internal_bits, void *stream);

/* Integer operands (what the EIGHTBIT / quantised builds do in hardware, MM.h:85-118): the codes of the w_qbits grids
 * as bytes.  codes[r][c] = clip(round(x / s + z)) - sgx_code_bias(is_signed, qbits), columns n_cols..ldc-1 = 0
 * (unsigned 8-bit codes 0..255 are stored minus 128; every other grid fits a signed byte as it is); value = code /
 * 2^(qbits-1) (1 bit: code / 2).  ldc a multiple of 16, codes 16-byte aligned for sgx_xw_dense_i8. */
int sgx_code_bias(int is_signed, int qbits);
int sgx_quantize_codes_i8(int is_signed, int qbits, float inv_scale, float zero, int n_rows, int n_cols, const float *x,
                          int64_t ldx, int8_t *codes, int64_t ldc, void *stream);
/* H[r][p] = requant( (sum_k Xc[r][k] Wc[p][k] + bias terms) / 2^(2(qbits-1)) ) on v_mfma_i32_16x16x64_i8: Xc unsigned
 * feature codes [n_rows][ldx], Wc signed weight codes in the layout of B, [P][ldw]; the epilogue is the fp32 form's
 * (shift by scale_fea, clip, decimal rounding; internal_bits = 0: none).  P <= 256.  workspace:
 * sgx_xw_dense_i8_workspace_bytes(P) bytes. */
size_t sgx_xw_dense_i8_workspace_bytes(int P);
int sgx_xw_dense_i8(int qbits, int n_rows, int M_fea, int P, const int8_t *Xc, int64_t ldx, const int8_t *Wc, int64_t ldw,
                    int scale_fea, int internal_bits, float *H, int64_t ldh, void *workspace, void *stream);

/* ---- the layer: replaces mmult_top / kernelmult1 (K.cpp:3762, :3969; KH:13-58) ------ */
typedef enum sgx_layer_order {
    SGX_ORDER_REFERENCE = 0,        /* D = act(A.(X.W))                                    */
    SGX_ORDER_AGGREGATE_FIRST = 1   /* D = act((A.X).W)                                    */
} sgx_layer_order;

/* The schedule of the layer's aggregate stage (sgx_layer_desc.schedule_adj). */
typedef enum sgx_layer_schedule_kind {
    SGX_SCHEDULE_DEFAULT = 0,       /* by rows: with plan_adj when one is given, without otherwise */
    SGX_SCHEDULE_FLAT = 1           /* by stored entries: "entry-split aggregation" below          */
} sgx_layer_schedule_kind;

typedef struct sgx_layer_desc {
    /* AXI-Lite scalars of the reference, same names (K.cpp:3777-3790, MMN cell 13) */
    int32_t gemm_mode;   /* 0: X is CSR (rowPtr_fea, columnIndex_fea, values_fea)
                            1: X is dense row-major [M_adj][M_fea] in values_fea; rowPtr_fea /
                               columnIndex_fea ignored (K.cpp:847-865, :985-1012)            */
    int32_t relu;        /* 1: D = max(D, 0) fused (K.cpp:2586-2590, :801-804)               */
    int32_t gat_mode;    /* 0: GCN aggregate  A.H ; 1: edge-softmax aggregate (SG.py:649-657) */
    int32_t N_adj;       /* rows of A and of D                                               */
    int32_t M_adj;       /* columns of A = rows of X                                         */
    int32_t M_fea;       /* columns of X = rows of W                                         */
    int32_t P_w;         /* columns of W and of D; any value >= 1 (no B_WIDTH_BLOCK tail rule) */
    int32_t bias_count;  /* must be 0; > 0 makes the reference preload and RETURN WITHOUT
                            COMPUTING (K.cpp:3876-3889) -- reproduced: D is left untouched    */
    int32_t dtype;       /* sgx_dtype                                                        */
    int32_t acc_mode;    /* sgx_acc_mode                                                     */
    int32_t spmm_block;  /* SPMM_BLOCK of the reference (MM.h:188); only observable in
                            SGX_ACC_REF_HALF (it fixes the partial-sum lane of each element);
                            0 means 1                                                        */
    int32_t gat_fill_dead_rows; /* gat_mode: what a row of A without a positive entry receives.
                            1: the mean of all rows of Wh -- the reference's dense emulation (its masked
                               row is constant, the softmax uniform over all N nodes, SG.py:638-641);
                            0: zero.  Equal whenever every row has a positive entry (self loops)   */

    /* buffers (device) -- the m_axi ports of K.cpp:3792-3828; the reference's four
     * aliases per port (rowPtr_fea1..4 etc., main_float.cpp:880-887) collapse to one */
    const void    *B;                 /* W^T  [P_w][M_fea]                          */
    void          *D;                 /* out  [N_adj][P_w]                          */
    const int32_t *rowPtr_fea;        /* [M_adj+1]            (gemm_mode 0)          */
    const int32_t *columnIndex_fea;   /* [nnz_fea]            (gemm_mode 0)          */
    const void    *values_fea;        /* [nnz_fea] or dense [M_adj*M_fea]            */
    const int32_t *rowPtr_adj;        /* [N_adj+1]                                   */
    const int32_t *columnIndex_adj;   /* [nnz_adj]                                   */
    const void    *values_adj;        /* [nnz_adj]                                   */

    /* GAT (gat_mode = 1): single head as in the reference (SG.py:1176-1178) */
    const void    *attention;         /* a [2*P_w]  (a1 = a[:P_w], a2 = a[P_w:]), same dtype */
    void          *E;                 /* optional out [nnz_adj] fp32: LeakyReLU(e_ij)        */
    void          *S;                 /* optional out [nnz_adj] fp32: softmax alpha_ij       */
    float          alpha;             /* LeakyReLU slope (SG.py:1172, default 0.2)           */
    /* FEA_THREADS / ADJ_THREADS of the reference (MM.h:166-167; 1, 2 or 4 there): each stage's rows
     * are cut into that many contiguous blocks -- rows/threads each, the remainder to the last
     * (K.cpp:3159-3164, :3517-3523) -- and the SPMM_BLOCK grouping restarts at every block.  Like
     * spmm_block only observable in SGX_ACC_REF_HALF; 0 means 1. */
    int32_t        fea_threads;
    int32_t        adj_threads;
    int32_t        gat_heads;         /* gat_mode: number of heads (see sgx_gat_aggregate); 0 means 1; the
                                         attention buffer then holds gat_heads vectors of 2*P_w/gat_heads */

    /* scratch in HBM for H = X.W (the reference's on-chip C tile, K.cpp:27) and split-row
     * partial sums; at least sgx_layer_workspace_bytes(desc) bytes, 256-byte aligned */
    void          *workspace;
    size_t         workspace_bytes;

    /* optional row schedules (see sgx_plan); NULL = none */
    const sgx_plan *plan_adj;
    const sgx_plan *plan_fea;

    /* optional profiling taps, the counterpart of the reference's profiling[] port
     * (K.cpp:3948-3962): hipEvent_t handles (as void*) recorded on `stream` right before and
     * right after the aggregation stage (A.H or GAT).  NULL = not recorded. */
    void *ev_agg_begin;
    void *ev_agg_end;

    /* optional: run the layer with the quantised arithmetic above (NULL = plain fp16/fp32 layer) */
    const sgx_quant *quant;

    /* sgx_layer_order.  The reference always forms H = X.W first (loop_fea feeds loop_adj, K.cpp:3629-3752).
     * With a dense X narrower than the output (M_fea < P_w: ogbn-products' 100 -> 256) aggregating first,
     * D = act((A.X).W), gathers M_fea instead of P_w columns per edge: the same sums in another association,
     * one rounding to the storage type in between as in the reference's order (Z = A.X in place of H).
     * Only gemm_mode 1, gat_mode 0, SGX_ACC_F32, no quant block; SGX_ERR_UNSUPPORTED otherwise.
     * A square dense fp16 layer (gemm_mode 1, M_fea = P_w = 64, GCN aggregate, SGX_ACC_F32, no quant block) runs as ONE
     * launch, the aggregation of X with W applied in its epilogue: D = act(f16(A.X).W), neither H nor Z in memory and no
     * workspace.  Under SGX_ORDER_AGGREGATE_FIRST that is bit-equal to the two launches.  SGX_ORDER_REFERENCE MAY apply W
     * after the aggregation for this shape too, and does: both associations gather 64 columns per edge, and the default
     * arithmetic is bound to the reference within a tolerance, not bit for bit (SGX_ACC_REF_HALF, which is, keeps the
     * reference's order).  The fused form needs a table below 4 GiB, X on a 4-byte boundary and a plan_adj that is
     * absent or neither cuts rows into tasks nor lists them in degree order; otherwise, or with
     * SGX_LAYER_NO_FUSED_DENSE set in the environment, the layer runs the staged launches of its order.
     * sgx_layer_workspace_bytes answers for the form the descriptor it is given will take: size the workspace with the
     * descriptor that runs, pointers and plans set. */
    int32_t order;

    /* Appended without a version bump (SGX_VERSION stays 110): both are 0 in a descriptor that was zeroed, and 0 is the
     * layer as it was.
     * schedule_adj: sgx_layer_schedule_kind.  Under SGX_SCHEDULE_FLAT the aggregate stage runs on the entry-split schedule
     * -- sgx_spmm_csr_flat (gat_mode 0) or sgx_gat_aggregate_flat (gat_mode 1, one head) -- with its scratch laid out
     * inside `workspace` (sgx_layer_workspace_bytes accounts for it at nnz_adj): no plan, nothing read back, nothing
     * allocated, every grid a function of the descriptor's host fields, so the whole layer records into a graph and replays
     * on another adjacency of the same capacity, whatever its rows are like.  The X.W stage runs as under the default
     * schedule (with plan_fea if one is given); the fused square dense fp16 form is not taken.
     * THE RULE: D is bit-equal to the X.W stage call (sgx_xw_dense, or sgx_transpose + sgx_xw_sparse, into an H whose
     * rows start on 16-byte boundaries, as the layer's own H does) followed by sgx_spmm_csr_flat / sgx_gat_aggregate_flat on the
     * same operands and the capacity nnz_adj; the statistics of sgx_layer_forward_stats are those of
     * sgx_gat_aggregate_flat(stats=).  Dead rows: gat_fill_dead_rows = 1 is that call's mean-row rule (fill NULL,
     * n_nodes = M_adj), 0 its zero rule (fill NULL, n_nodes = 0).
     * SGX_ERR_UNSUPPORTED, before any launch, for SGX_SCHEDULE_FLAT together with any of: plan_adj != NULL, quant != NULL,
     * acc_mode != SGX_ACC_F32, gat_heads > 1, E or S outputs, SGX_ORDER_AGGREGATE_FIRST; and for a schedule_adj that is
     * neither enumerator.  nnz_adj < 0 (or above INT32_MAX): SGX_ERR_SHAPE.
     * nnz_adj: the entries columnIndex_adj / values_adj hold -- a capacity, a bound on rowPtr_adj[N_adj], as `nnz` in the
     * entry-split calls.  Read only under SGX_SCHEDULE_FLAT.
     * Quantised layer on the entry-split schedule (added without a version bump: one new flag, two new declarations):
     * `quant != NULL` is accepted under SGX_SCHEDULE_FLAT when, and only when, quant->flags carries SGX_QUANT_FLAT; without
     * the bit the answer stays SGX_ERR_UNSUPPORTED.  The other refusals above hold with the bit set (plan_adj, gat_heads > 1,
     * E / S, SGX_ORDER_AGGREGATE_FIRST; dtype and acc_mode as for every quantised layer).  The quantised copies of B, X, A
     * (skipped under SGX_QUANT_ADJ_DONE; quant->nnz_adj entries, which may be the capacity) and the attention vector are
     * made as under the default schedule, and stage 1 runs as there with its requantising epilogue (the dense fp32 form,
     * the int8 form under SGX_QUANT_INT8[_AUTO], a CSR X by rows with plan_fea).  Stage 2 is sgx_spmm_csr_flat_ep /
     * sgx_gat_aggregate_flat_ep with out_scale = quant->deq_factor on the quantised operands.  The workspace is the default
     * schedule's quantised layout followed, on a 256-byte boundary, by the entry-split scratch at nnz_adj.
     * THE RULE: D, and the statistics of sgx_layer_forward_stats, are bit-equal to those named stage calls composed on the
     * same operands and capacity (sgx_fake_quantize / sgx_quantize_codes_i8, the X.W stage + sgx_requantize or
     * sgx_xw_dense_i8, then the _ep call).  sgx_layer_schedule answers 2. */
    int32_t schedule_adj;
    int64_t nnz_adj;
} sgx_layer_desc;

size_t sgx_layer_workspace_bytes(const sgx_layer_desc *desc);
int    sgx_layer_forward(const sgx_layer_desc *desc, void *stream);
/* Which schedule the aggregate stage of sgx_layer_forward / sgx_layer_forward_stats takes for this descriptor, for reports
 * and tests (added without a version bump: a new declaration): a host query without a launch that reads no device
 * memory, answered by the checks the call itself makes.  0 = by rows without a plan, 1 = by rows with plan_adj,
 * 2 = entry-split; negative = the sgx_status the call would return for the descriptor's modes and shapes. */
int    sgx_layer_schedule(const sgx_layer_desc *desc);

/* ---- the stages, individually (the dataflow processes of K.cpp:3629-3752) ---------- */

/* A.H aggregation = loop_adj / compute2 / writec (K.cpp:3339, :2483, :713):
 *   D[r][0:n_feat] = act( sum_e values[e] * H[columnIndex[e]][0:n_feat] ),  r in [0,n_rows)
 * H is [n_cols][ldh], D is [n_rows][ldd] (leading dimensions in elements).  Rows of H that start on
 * a dword (H 4-byte aligned, ldh*sizeof(elem) a multiple of 4) are gathered 16 bytes per lane; rows on
 * odd halves -- and, for tables of 4 GiB and more, rows that are not 16-byte aligned -- one element per
 * lane.  Fastest when no row straddles a 128-byte line (ldh*sizeof(elem) a multiple of 128, or a power
 * of two below it).  scratch/scratch_bytes: needed only when `plan` has long rows
 * (sgx_spmm_scratch_bytes). */
int sgx_spmm_csr(int dtype, int acc_mode, int spmm_block, int relu,
                 int n_rows, int n_cols, int n_feat,
                 const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                 const void *H, int64_t ldh, void *D, int64_t ldd,
                 const sgx_plan *plan, void *scratch, size_t scratch_bytes, void *stream);
size_t sgx_spmm_scratch_bytes(const sgx_plan *plan, int n_feat);

/* The same aggregation in two passes over disjoint edge sets, for the multi-GPU path (the edges
 * whose column lives in the rank's own partition while the halo rows travel over xGMI, then the
 * halo edges): pass 1 writes the fp32 sums to acc_out (D = NULL), pass 2 starts from acc_in and
 * writes D = act(acc_in + A.H).  acc_* are [n_rows][ld_acc] fp32; either may be NULL. */
int sgx_spmm_csr_acc(int dtype, int relu, int n_rows, int n_cols, int n_feat,
                     const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                     const void *H, int64_t ldh, void *D, int64_t ldd,
                     const float *acc_in, float *acc_out, int64_t ld_acc,
                     const sgx_plan *plan, void *scratch, size_t scratch_bytes, void *stream);

/* ---- entry-split aggregation ----------------------------------------------------------------------------
 * sgx_spmm_csr's contract in SGX_ACC_F32 arithmetic (fp16 or fp32 storage, fp32 products and sums, one rounding on
 * the store) on a schedule that depends on the stored-entry count alone: no plan, nothing read back, nothing allocated,
 * no synchronisation, the grids a function of `nnz` -- so the call records into a graph and replays on other matrices
 * of the same capacity -- and balanced on any degree distribution, because the work is cut by stored entries, not by rows.
 *
 * Ownership rule, with T = sgx_spmm_flat_chunk() and end = rowPtr[n_rows] as the device reads it:
 *   - the stored entries are cut into chunks of T consecutive entries, chunk c = entries [cT, min((c+1)T, end)), one
 *     wavefront per chunk; a chunk finds its first row by a search in rowPtr on the device;
 *   - a row that lies wholly inside one chunk is summed and stored by that chunk;
 *   - a row that crosses a chunk end leaves one fp32 partial row per chunk it touches in `scratch`;
 *   - the chunk that holds a crossing row's first entry is its leader: in a second launch, whose grid is again a
 *     function of the chunk count only, the leader adds the row's partials in chunk order and stores the row once;
 *   - an empty row belongs to the chunk that holds entry index rowPtr[r]; if that index equals end, to the last chunk;
 *     for end == 0 a single degenerate chunk owns all rows.  It is stored as act(0), which is +0.
 * Every row of D is therefore written exactly once, by plain vector stores and without atomics, and the order in which
 * a row is summed depends only on rowPtr and T (and the call's operand layout): two runs give the same bits.  A row
 * of fewer than 64 entries inside one chunk gets the bits sgx_spmm_csr gives it without a plan.
 *
 * nnz is a host argument and may be a capacity: a bound on rowPtr[n_rows] (and no more than columnIndex / values
 * hold).  Chunks that start at or past the real end do nothing; empty rows are assigned by the real end.
 * H is gathered as by sgx_spmm_csr (16 bytes per lane where rows start on a dword, one element per lane on odd
 * halves, range-checked buffer loads, any n_feat >= 1); tables of 4 GiB and more: SGX_ERR_UNSUPPORTED -- the form is
 * for batch-sized matrices.  scratch: sgx_spmm_flat_scratch_bytes(nnz, n_feat) bytes (never 0 for valid arguments; 0
 * for nnz < 0, nnz > INT32_MAX or n_feat < 1), 256-byte aligned, needed by every call.
 * Argument errors, returned before anything is launched: a negative size, n_feat < 1, ldh or ldd below n_feat, nnz
 * outside [0, INT32_MAX]: SGX_ERR_SHAPE; a dtype other than SGX_F16 / SGX_F32: SGX_ERR_UNSUPPORTED; (n_rows == 0:
 * SGX_OK;) rowPtr or D NULL, columnIndex or values NULL with nnz > 0, H NULL with nnz > 0 and n_cols > 0:
 * SGX_ERR_NULL; a table past 32-bit byte offsets: SGX_ERR_UNSUPPORTED; scratch NULL or too small: SGX_ERR_WORKSPACE;
 * scratch off a 256-byte boundary, an index array off 4 bytes, values, H or D off an element: SGX_ERR_ALIGN. */
int    sgx_spmm_flat_chunk(void);
size_t sgx_spmm_flat_scratch_bytes(int64_t nnz, int n_feat);
int    sgx_spmm_csr_flat(int dtype, int relu, int n_rows, int n_cols, int n_feat, int64_t nnz,
                         const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                         const void *H, int64_t ldh, void *D, int64_t ldd,
                         void *scratch, size_t scratch_bytes, void *stream);
/* The same call with the quantised layer's store epilogue (added without a version bump: a new declaration;
 * sgx_spmm_csr_flat is this call with the epilogue off, and the scratch is the same size).
 *   out_scale         0 = off; otherwise every element of D is multiplied by it after the activation (deq_o, SG.py:666-667)
 *   rq_internal_bits  0 = no requantisation (rq_scale_fea is then not read); otherwise the H-stage rule of the quantised
 *                     layer, round_decimals(clip(x / 2^rq_scale_fea, +-(2^ib - 1) / 2^ib), ib - 1), before the activation.
 *                     rq_scale_fea outside [0, 30], rq_internal_bits outside [1, 30], or a dtype other than SGX_F32 when
 *                     requantising: SGX_ERR_UNSUPPORTED, before anything is launched.
 * The partial rows of a crossing row stay raw fp32 sums; the epilogue acts exactly once per element of D, on the store of
 * a finished row -- inside a chunk, after the cooperative walk, or in the second launch.
 * THE RULE (dtype SGX_F32: every step is one IEEE operation, so it holds bit for bit): with out_scale = s, D equals
 * sgx_spmm_csr_flat's D times s in fp32; with requantisation, D equals sgx_requantize applied to sgx_spmm_csr_flat's D
 * (the rule is odd and maps 0 to 0, so it commutes with the ReLU); with both, the requantised D times s.
 * dtype SGX_F16: the rule of the row kernels (sgx_epilogue in the library: "fp16 instantiations ignore it") -- out_scale
 * is NOT applied, D equals sgx_spmm_csr_flat's bit for bit.  The quantised layer is fp32-only. */
int    sgx_spmm_csr_flat_ep(int dtype, int relu, int n_rows, int n_cols, int n_feat, int64_t nnz,
                            const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                            const void *H, int64_t ldh, void *D, int64_t ldd,
                            void *scratch, size_t scratch_bytes, float out_scale, int rq_scale_fea, int rq_internal_bits,
                            void *stream);

/* X.W with dense X = loop_fea / compute1 in gemm_mode 1 (K.cpp:2932, :2605, :847-865),
 * on the matrix cores:  H[r][0:P] = sum_k X[r][k] * Wt[p][k].
 * X [n_rows][ldx], Wt [P][ldw] (= B), H [n_rows][ldh]; columns P..ldh-1 of H are zeroed. */
int sgx_xw_dense(int dtype, int acc_mode, int spmm_block, int n_rows, int M_fea, int P,
                 const void *X, int64_t ldx, const void *Wt, int64_t ldw,
                 void *H, int64_t ldh, void *stream);

/* The same product with the activation on its stores, D = act(X.Wt^T): the second stage of
 * SGX_ORDER_AGGREGATE_FIRST (X := A.X) for callers that run the stages themselves (the multi-GPU exchange of
 * sgracex1_amd/dist.py).  fp32-accumulate arithmetic only; pad columns P..ldh-1 are zeroed. */
int sgx_xw_dense_act(int dtype, int relu, int n_rows, int M_fea, int P,
                     const void *X, int64_t ldx, const void *Wt, int64_t ldw,
                     void *H, int64_t ldh, void *stream);

/* Which kernel arm sgx_xw_dense / sgx_xw_dense_act take for these operands, for reports and tests (added without a version
 * bump, SGX_VERSION stays 110: a new declaration, nothing else changes): a host query without a launch and without a
 * device (where the launch would fall back to 256 CUs the query does too), answered by the functions the launch itself
 * uses.  X, Wt, H: the pointers the call would get (only their alignment is read; non-NULL when n_rows > 0); pitches in
 * elements.  Returns the negative sgx error the call would return before a launch, or
 *   kind | a << 4 | b << 10 | vec << 16 | wgs_per_cu << 17 | blocks << 21 | waves << 32
 * in fields of 4 (kind), 6 (a), 6 (b), 1 (vec), 4 (wgs_per_cu), 11 (blocks) and 31 (waves) bits: the SGX_XW_FORM_*_SHIFT and
 * _MASK constants below, field = word >> SHIFT & MASK.
 * kind    a, b      blocks                                waves
 * TILE       NT, MT    column blocks of 256 (a, b: the LAST  wavefronts of one block's launch: one tile of 16 MT rows
 *                      block's; whole ones before it are      each, never more
 *                      <16, 1>, or <16, 2> from 32768 rows)
 * STATIONARY KS, NTW   column groups of 16 NTW columns        wavefronts the persistent grid holds (whole workgroups of
 *            (fp32:                                           four): the kernel makes waves / blocks (rounded down)
 *            KB, NTW)                                         streams of them, stream s walks row tiles s, s + streams,
 *                                                             ... of 32 rows (fp32: 16); waves % blocks wavefronts idle
 * TILE_LDS   8, 8      column blocks of 128                  wavefronts of the grid (four per 128 x 128 tile)
 * WLDS       fp16: NT, n_cb; fp32: KB and the LAST block's NT (whole blocks before it: 16)
 *                      fp16: column blocks of 16 NT          fp16: per column block, wavefront w walks row tiles
 *                      columns (one grid); fp32: blocks      w, w + waves, ... of 32 rows; fp32: of one block's launch,
 *                      of 256 (one launch each)              tiles of 16 rows
 * REF_HALF   0, 0      0                                     0   (SGX_ACC_REF_HALF: its arms are refhalf.hip's own)
 * NONE       n_rows == 0: nothing is launched
 * vec = 1: H is stored by vectors (16 bytes: fp32, fp16 STATIONARY with NTW even, fp16 WLDS; 8 bytes otherwise), 0: element
 * by element (H or its pitch under-aligned).  wgs_per_cu: workgroups a CU is given by the persistent grids (STATIONARY,
 * WLDS), 0 otherwise.  blocks saturates at 2047. */
#define SGX_XW_FORM_NONE 0
#define SGX_XW_FORM_TILE 1
#define SGX_XW_FORM_STATIONARY 2
#define SGX_XW_FORM_TILE_LDS 3
#define SGX_XW_FORM_WLDS 4
#define SGX_XW_FORM_REF_HALF 5
#define SGX_XW_FORM_KIND_MASK 15
#define SGX_XW_FORM_A_SHIFT 4
#define SGX_XW_FORM_A_MASK 63
#define SGX_XW_FORM_B_SHIFT 10
#define SGX_XW_FORM_B_MASK 63
#define SGX_XW_FORM_VEC_SHIFT 16
#define SGX_XW_FORM_WGS_SHIFT 17
#define SGX_XW_FORM_WGS_MASK 15
#define SGX_XW_FORM_BLOCKS_SHIFT 21
#define SGX_XW_FORM_BLOCKS_MASK 2047
#define SGX_XW_FORM_WAVES_SHIFT 32
int64_t sgx_xw_dense_form(int dtype, int acc_mode, int n_rows, int M_fea, int P, const void *X, int64_t ldx,
                          const void *Wt, int64_t ldw, const void *H, int64_t ldh);

/* X.W with CSR X = loop_fea / compute1 in gemm_mode 0 (K.cpp:1960-2078).
 * W_rowmajor is [M_fea][ldw] (use sgx_transpose to get it from B). */
int sgx_xw_sparse(int dtype, int acc_mode, int spmm_block, int n_rows, int M_fea, int P,
                  const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                  const void *W_rowmajor, int64_t ldw, void *H, int64_t ldh,
                  const sgx_plan *plan, void *scratch, size_t scratch_bytes, void *stream);

/* out[c][r] = in[r][c]; in [rows][ldi], out [cols][ldo]; pads out columns rows..ldo-1 with 0.
 * The weight-tile load B_accel[i][j] = B[i + j*M_fea] (K.cpp:3038-3051). */
int sgx_transpose(int dtype, int rows, int cols, const void *in, int64_t ldi,
                  void *out, int64_t ldo, void *stream);

/* GAT aggregation on an already computed Wh (SG.py:309-314, :634-661), single head:
 *   e_ij = LeakyReLU_alpha(Wh_i.a1 + Wh_j.a2) for stored edges with values[e] > 0 (the stored value as stored: +0.0 and
 *   -0.0 are masked, positive fp16 and fp32 subnormals are live; every form and the backward edge pass test it so),
 *   alpha_ij = softmax_j(e_ij),  D_i = act(sum_j alpha_ij Wh_j).
 * Wh has n_cols rows; row r of the adjacency is node r of Wh (n_rows <= n_cols: the reference's
 * square case is n_rows == n_cols, a rank of the partitioned graph passes its own rows first and
 * the halo rows behind them).
 * fill_dead_rows: see sgx_layer_desc.gat_fill_dead_rows.  s_scratch: sgx_gat_scratch_bytes() bytes
 * (the per-node scores Wh.a1, Wh.a2 and the column-mean partials).  E/S optional [nnz] fp32.
 * n_heads > 1 (BASELINE config 5; the reference itself has one head, SG.py:1176-1178): the formula
 * above on each slice of n_feat / n_heads columns with its own vector attention[h][0 : 2*F_head],
 * outputs concatenated -- what n_heads single-head calls on the slices give; E/S are [nnz][n_heads].
 * plan (optional): rows it marks long are cut into edge chunks with per-chunk softmax states that are
 * merged in a fixed order.  With a plan (which tells the stored-entry count) the aggregate runs in two stages -- the
 * softmax weights on the edges, then the A.H aggregation with those weights; sgx_gat_scratch_bytes then includes
 * nnz * n_heads floats for the weights (S takes them when given). */
size_t sgx_gat_scratch_bytes(int n_cols, int n_feat, int n_heads, int fill_dead_rows, const sgx_plan *plan);
int sgx_gat_aggregate(int dtype, int relu, int fill_dead_rows, int n_rows, int n_cols, int n_feat, int n_heads,
                      float alpha,
                      const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                      const void *Wh, int64_t ldh, const void *attention,
                      void *D, int64_t ldd, float *E, float *S, const sgx_plan *plan, float *s_scratch,
                      void *stream);

/* The same aggregate for one rank of a node-partitioned graph: a row without a live edge receives `fill`
 * (fp32 [n_feat], device) -- the mean of the rows of Wh of ALL n_nodes nodes, which the caller reduces across ranks
 * (sgx_col_sums per rank, one all-reduce of n_feat floats) -- and S = 1/n_nodes on its stored edges: the reference's
 * uniform softmax over every node (SG.py:638-641), which one rank's table (own rows + halo rows) cannot give.
 * fill = NULL: such rows give 0.  Scratch: sgx_gat_scratch_bytes(n_cols, n_feat, n_heads, 0, plan). */
int sgx_gat_aggregate_fill(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha,
                           const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                           const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd, float *E, float *S,
                           const float *fill, int64_t n_nodes, const sgx_plan *plan, float *s_scratch, void *stream);
/* out[j] = sum over rows of X[r][j], fp32, slab sums added in a fixed order (bitwise reproducible).
 * scratch: sgx_col_sums_scratch_bytes(n_feat) bytes. */
size_t sgx_col_sums_scratch_bytes(int n_feat);
int sgx_col_sums(int dtype, int n_rows, int n_feat, const void *X, int64_t ldx, float *out, float *scratch, void *stream);

/* ---- helpers on either side of the path (SURVEY 8f "next" rows) -------------------- */

/* Checks rowPtr[0]==0, monotone, rowPtr[n_rows]==nnz and 0 <= columnIndex < n_cols on the
 * device.  Synchronises the stream.  Returns SGX_OK or SGX_ERR_CSR. */
int sgx_csr_validate(const int32_t *rowPtr, const int32_t *columnIndex, int n_rows, int n_cols,
                     int64_t nnz, void *stream);

/* COO (row index per edge, sorted by row) -> CSR row pointer; the GAT bitstream is fed COO
 * (SG.py:1222, :1245).  rowPtr [n_rows+1]. */
int sgx_coo_to_csr(const int32_t *rowIndex, int64_t nnz, int n_rows, int32_t *rowPtr, void *stream);

/* Weight gradient of the layer's backward pass, grad_W = X^T . G with G = adj @ grad_output already
 * aggregated by sgx_spmm_csr (FPYNQ.backward, MOL cell 16; the reference runs it in torch on the CPU).
 * X [n_rows][ldx] fp16|fp32 dense, G [n_rows][ldg] fp32, out [M][ldo] fp32 (exact fp32 fma chains,
 * slab sums added in a fixed order).  Columns P .. ldo-1 of out are not written; n_rows = 0 clears
 * out[M][P] and reads neither X nor G (both may be NULL), and sgx_xt_g_workspace_bytes(0, M, P) is a
 * valid, non-zero size.  The other two products of the backward pass are existing entry points:
 * adj @ g = sgx_spmm_csr, grad_x = G . W^T = sgx_xw_dense(G, Wt := W [M][P]); for a CSR X,
 * X^T . G = sgx_spmm_csr over the CSR of X^T. */
size_t sgx_xt_g_workspace_bytes(int n_rows, int M, int P);
int sgx_xt_g(int dtype_x, int n_rows, int M, int P, const void *X, int64_t ldx, const float *G, int64_t ldg,
             float *out, int64_t ldo, void *workspace, size_t workspace_bytes, void *stream);

/* Edge pass of the GAT layer's backward (FPYNQ_GAT.backward, SG.py:884-1126, on the stored edges instead
 * of dense N x N matrices): with E, S the forward's per-edge outputs, G = grad_output [n_rows][ldg] and
 * Wh [n_cols][ldw], all fp32,
 *   d_e = G[row e] . Wh[col e];  dx_e = S_e d_e;  sg_e = dx_e - S_e sum_row(dx);
 *   sg_e = 0 where values[e] <= 0;  sg_e *= (E_e > 0 ? 1 : alpha)
 * writes sg [nnz] and g1[r] = sum_row(sg).  The attention gradient is then [Wh^T g1 ; Wh^T g2] with
 * g2 = the column sums of sg (row sums over A^T: sgx_spmm_csr) through sgx_xt_g.
 * dead, dead_row_sum (both NULL, or both [n_rows]): rows with dead[r] != 0 are the rows the forward found
 * without a positive entry, whose softmax is uniform over ALL n_cols columns (SG.py:638-641); for them
 * sum_row(dx) is dead_row_sum[r] = G[r] . colsum(Wh) / n_cols instead of the sum over the stored entries. */
int sgx_gat_backward_edges(int dtype_values, int n_rows, int n_cols, int n_feat, float alpha,
                           const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                           const float *E, const float *S, const float *G, int64_t ldg, const float *Wh, int64_t ldw,
                           const uint8_t *dead, const float *dead_row_sum, float *sg, float *g1, void *stream);

/* ---- the GAT aggregate and its backward from row softmax statistics instead of E and S -----------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * E and S (2 nnz n_heads floats) are redundant: four small arrays hold what forms them again,
 *     E_e = LeakyReLU_alpha(fp32(score_row[i] + score_col[c]))          stored entry e = (i, c), per head
 *     live iff values[e] > 0, the stored value as stored (see sgx_gat_aggregate)
 *     S_e = exp(E_e - row_max[i]) / row_sum[i]   on a live entry,   0 on a masked one
 * A row without a live entry (a dead row) has row_max = 0 and row_sum = 0; S_e on each of its stored entries is the
 * constant of the dead-row rule in force: 1/n_cols (fill_dead_rows), 1/n_nodes (sgx_gat_aggregate_fill) or 0, which the
 * calls that read the statistics take as `dead_weight`.  Every call below forms E_e and S_e by exactly this expression
 * (fp32 add, expf, one division), so they agree bit for bit among themselves.  All four arrays are required together. */
typedef struct sgx_gat_stats {      /* all fp32, device */
    float *score_row;   /* [n_rows][n_heads]  Wh_i . a1 of the head               */
    float *score_col;   /* [n_cols][n_heads]  Wh_c . a2 of the head               */
    float *row_max;     /* [n_rows][n_heads]  m_i: max of the row's LIVE scores   */
    float *row_sum;     /* [n_rows][n_heads]  l_i: sum over live e of exp(E_e-m_i) */
} sgx_gat_stats;

/* sgx_gat_aggregate / sgx_gat_aggregate_fill without the E / S outputs, delivering the statistics.  D is formed by the
 * very launches of those calls with E = S = NULL -- the one walk (gat_fused.hip) wherever they take it, the two stages or
 * the one-pass kernels elsewhere -- so D is bit-equal to theirs on the same arguments.  The statistics come from the
 * scores of the aggregate's pre-pass (s_scratch) and one more pass over the stored entries that moves no row of Wh (4-byte
 * score gathers; rows over 256 entries by a whole workgroup): the (max, sum) of each row's live scores, the sum in the
 * order of that pass.  The one walk forms a neighbour's score from the row it gathers, so the weights it used may differ
 * from the S_e of the statistics in the last bits -- inside the error bound of either.
 * Dead-row rule: fill != NULL -- the partitioned rule of sgx_gat_aggregate_fill (n_nodes >= 1); fill == NULL and
 * n_nodes == 0 -- dead rows give 0 (fill_dead_rows = 0); fill == NULL and n_nodes == n_cols > 0 -- the mean of the rows
 * of Wh (fill_dead_rows = 1); fill == NULL with any other n_nodes: SGX_ERR_SHAPE.  Scratch: sgx_gat_scratch_bytes with the
 * fill_dead_rows of the rule (0 with a fill row).  stats or one of its members NULL: SGX_ERR_NULL, n_cols * n_heads * 4
 * bytes of scores beyond 32-bit offsets: SGX_ERR_UNSUPPORTED; both before anything is launched. */
int sgx_gat_aggregate_stats(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha,
                            const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                            const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd,
                            const float *fill, int64_t n_nodes, const sgx_plan *plan, float *s_scratch,
                            const sgx_gat_stats *stats, void *stream);

/* sgx_layer_forward for gat_mode = 1 with desc->E == desc->S == NULL, delivering the statistics of its aggregate (of the
 * quantised operands when desc->quant is set: whatever the forward used).  D is bit-equal to sgx_layer_forward's on the
 * same descriptor; the workspace is the same (sgx_layer_workspace_bytes).  gat_mode = 0, or E / S set:
 * SGX_ERR_UNSUPPORTED; stats or a member NULL: SGX_ERR_NULL. */
int sgx_layer_forward_stats(const sgx_layer_desc *desc, const sgx_gat_stats *stats, void *stream);

/* E and / or S [nnz][n_heads] fp32 formed from the statistics (either may be NULL): the side outputs after a forward
 * that did not write them.  dtype_values: the element type of `values`. */
int sgx_gat_edge_outputs(int dtype_values, int n_rows, int n_cols, int n_heads, float alpha,
                         const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                         const sgx_gat_stats *stats, float dead_weight, float *E, float *S, void *stream);

/* sgx_gat_backward_edges with the statistics in place of E and S: the dots kernel forms S_e from score_row[row],
 * score_col[col] (a 4-byte range-checked gather), row_max and row_sum instead of loading it, the row kernels take the
 * LeakyReLU slope from the E_e they form again.  S_out (optional, [nnz]) receives S_e: the attention matrix the caller
 * multiplies with next.  One head: the statistics are [n_rows] / [n_cols] arrays (n_heads = 1; more: SGX_ERR_UNSUPPORTED).
 * dead / dead_row_sum as in sgx_gat_backward_edges; dead_weight: S_e of the stored entries of a row whose row_sum is 0. */
int sgx_gat_backward_edges_stats(int dtype_values, int n_rows, int n_cols, int n_feat, int n_heads, float alpha,
                                 const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                 const sgx_gat_stats *stats, float dead_weight, const float *G, int64_t ldg,
                                 const float *Wh, int64_t ldw, const uint8_t *dead, const float *dead_row_sum,
                                 float *sg, float *g1, float *S_out, void *stream);

/* ---- entry-split GAT aggregate ---------------------------------------------------------------------------
 * Added without a version bump: both declarations are new.  The counterpart of "entry-split aggregation" above; it stands
 * here because it takes the sgx_gat_stats declared in this section.
 * sgx_gat_aggregate's arithmetic for ONE head on the schedule of sgx_spmm_csr_flat: D_i = act(sum over live e of S_e Wh_c), with the
 * score formed as the statistics form it ("from row softmax statistics" above): E_e = LeakyReLU_alpha(fp32(score_row[i] +
 * score_col[c])), an entry live iff values[e] > 0 as stored, S_e = exp(E_e - m_i) / l_i.  No plan, nothing read back,
 * nothing allocated, no synchronisation, the grids a function of `nnz`: the call records into a graph and replays on other
 * matrices of the same capacity.  n_heads != 1 (0 counts as 1): SGX_ERR_UNSUPPORTED.  There are no E / S outputs.
 *
 * The ownership rule is sgx_spmm_csr_flat's, unchanged (T = sgx_spmm_flat_chunk(), one wavefront per chunk, two searches
 * in rowPtr, head slot 2k / tail slot 2c + 1, the empty rows, nnz as a capacity).  What a piece leaves is a running
 * softmax state (m, l, acc[n_feat]) in fp32: m the maximum of the live scores seen, l the sum of exp(E_e - m) over them,
 * acc the weighted row, rescaled when m moves; a piece without a live entry is (-inf, 0, 0).
 *   - a row wholly inside one chunk is normalised (acc / l) and stored by that chunk;
 *   - a crossing row's leader merges its states in chunk order in the second launch: M = max m_k, l = sum l_k exp(m_k - M),
 *     acc = sum acc_k exp(m_k - M), and stores the row once; a state with m_k = -inf contributes nothing, also when
 *     M = -inf -- that row is dead.
 * Every row of D is written exactly once, by plain stores and without atomics; the order of every sum depends on rowPtr,
 * T and the operand layout only: two runs give the same bits.
 * Dead rows (no live entry, l = 0), by the rule of sgx_gat_aggregate_stats: fill != NULL -- the row `fill` [n_feat] fp32
 * (n_nodes >= 1); fill == NULL and n_nodes == 0 -- 0; fill == NULL and n_nodes == n_cols -- the mean row of Wh, formed in
 * the scratch by the column-sum pre-pass in a fixed order; fill == NULL with any other n_nodes: SGX_ERR_SHAPE.
 * stats is optional: NULL -- nothing is written; otherwise all four members are required, score_row / score_col receive
 * the pre-pass's scores (those of sgx_gat_aggregate without a plan, bit for bit), row_max / row_sum the merged m and l, or
 * 0 and 0 on a dead row, written by whoever stores the row.  sgx_gat_edge_outputs and sgx_gat_backward_edges_stats work on
 * them as they are.
 * scratch: sgx_gat_flat_scratch_bytes(nnz, n_rows, n_cols, n_feat, mean_rule) bytes, mean_rule != 0 for the mean-row rule;
 * monotone in nnz, never 0 for valid arguments (0 for nnz outside [0, INT32_MAX], n_rows < 0, n_cols < n_rows, n_feat < 1);
 * 256-byte aligned, needed by every call.  Row r of the adjacency is node r of Wh (n_rows <= n_cols).
 * Argument errors, all returned before anything is launched: the dead-row rule's; a negative size, n_cols < n_rows,
 * n_feat < 1, ldh or ldd below n_feat, nnz outside [0, INT32_MAX]: SGX_ERR_SHAPE; n_heads != 1, a dtype other than SGX_F16 /
 * SGX_F32: SGX_ERR_UNSUPPORTED; (n_rows == 0: SGX_OK;) rowPtr, D, Wh or attention NULL, columnIndex or values NULL with
 * nnz > 0, a member of a given stats NULL: SGX_ERR_NULL; a table past 32-bit byte offsets: SGX_ERR_UNSUPPORTED; scratch
 * NULL or too small: SGX_ERR_WORKSPACE; scratch off a 256-byte boundary, an index array or fill off 4 bytes, values, Wh,
 * attention or D off an element: SGX_ERR_ALIGN. */
size_t sgx_gat_flat_scratch_bytes(int64_t nnz, int n_rows, int n_cols, int n_feat, int mean_rule);
int    sgx_gat_aggregate_flat(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha, int64_t nnz,
                              const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                              const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd,
                              const float *fill, int64_t n_nodes, void *scratch, size_t scratch_bytes,
                              const sgx_gat_stats *stats, void *stream);
/* The same call with the quantised layer's deq_o on its stores (added without a version bump: a new declaration;
 * sgx_gat_aggregate_flat is this call with out_scale = 0, which means off, and the scratch is the same size).  The running
 * softmax states in the slots stay raw fp32; out_scale multiplies every element of a finished row exactly once, after the
 * normalisation -- or the dead row's value under each of the three dead-row rules -- and after the activation, as the row
 * kernels of sgx_layer_forward apply it.  THE RULE (SGX_F32): D equals sgx_gat_aggregate_flat's D times out_scale in fp32,
 * bit for bit, and the statistics are unchanged.  SGX_F16: out_scale is not applied (the row kernels' rule). */
int    sgx_gat_aggregate_flat_ep(int dtype, int relu, int n_rows, int n_cols, int n_feat, int n_heads, float alpha, int64_t nnz,
                                 const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                                 const void *Wh, int64_t ldh, const void *attention, void *D, int64_t ldd,
                                 const float *fill, int64_t n_nodes, void *scratch, size_t scratch_bytes,
                                 const sgx_gat_stats *stats, float out_scale, void *stream);

/* Readout + classifier head of the graph-classification model (MOL cell 18 tail) in one launch:
 * pooled[g][:] = mean of X rows [graph_ptr[g], graph_ptr[g+1])  (global_mean_pool over a sorted
 * `batch` vector), logits[g][c] = bias[c] + W[c][:] . pooled[g][:]  (torch Linear, W [C][F] fp32).
 * pooled or logits may be NULL (then W, bias are not read); bias may be NULL. */
int sgx_readout_mean_linear(int dtype, int n_graphs, int F, int C, const void *X, int64_t ldx,
                            const int32_t *graph_ptr, const float *W, const float *bias, float *pooled,
                            float *logits, void *stream);

/* Backward of that pooling for the training step (the autograd of global_mean_pool in MOL cell 18's forward, cell 20's
 * loop): grad_X[r][:] = dtype(grad_pooled[g][:] * (1 / (graph_ptr[g+1] - graph_ptr[g]))) for the rows r of graph g -- the
 * fp32 reciprocal of the graph's size rounded once, the fp32 product, then `dtype` (the element type of the layer output
 * the pooling read); rows outside every graph and columns F .. ldg-1 are not written. */
int sgx_readout_mean_backward(int dtype, int n_graphs, int F, const float *grad_pooled, const int32_t *graph_ptr,
                              void *grad_X, int64_t ldg, void *stream);

/* ReLU backward of RPYNQ (MOL cell 16): grad[i] = (out[i] == 0) ? 0 : grad[i], in place. */
int sgx_relu_mask_backward(int dtype_out, const void *out, int dtype_grad, void *grad, int64_t n,
                           void *stream);

/* dst[i][0:n_feat] = src[row_index[i]][0:n_feat], i in [0, n_rows): the pack step of the halo exchange between the
 * GPUs of a node -- the rows of H a peer's edges reference, gathered into the send buffer of the all-to-all (the
 * block select of dsp_kernel_float_adj_4, K.cpp:217-264, done on the sending side).  ld_* in elements. */
int sgx_pack_rows(int dtype, int64_t n_rows, int n_feat, const void *src, int64_t ld_src, const int32_t *row_index,
                  void *dst, int64_t ld_dst, void *stream);

/* ---- neighbour sampling for mini-batch training ---------------------------------------
 * The NeighborLoader batches of the reference's demo (demo/emulation/demo_sgrace.py:112-125, `full_graph = 0`:
 * num_neighbors=[10], batch_size=128, input_nodes=train_mask), sampled on the device (csrc/sample.hip).
 *
 * Graph: the CSR (rowPtr [n_nodes+1], columnIndex [nnz]) built on the TARGET of every edge, so row v holds the
 * in-edges j -> v (PyG's flow="source_to_target").  Self loops and repeated edges are positions like any other.
 *
 * Sampling rule, for seed / frontier node v of degree deg = rowPtr[v+1] - rowPtr[v] at hop h with fan-out k:
 *   - k == -1 or deg <= k: every position 0 .. deg-1;
 *   - otherwise a uniform k-subset of the positions without replacement, by Floyd's algorithm:
 *       S = {};  for j = deg-k .. deg-1:  t = draw(j);  S += (t in S) ? j : t;
 *   - the positions of S in ascending order.
 * The draw is a counter-based hash; mix64 is the splitmix64 finaliser
 *     z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  z ^ (z >> 31)
 * on uint64 with wrap-around, and
 *     key_h   = mix64(mix64(mix64(seed) ^ step) ^ (uint64)h)          h = hop index, 0 = the hop that samples the seeds
 *     w       = ((uint64)(uint32)v << 32) | (uint32)j                 node id in bits 63..32, Floyd index in 31..0
 *     draw(j) = (mix64(key_h ^ mix64(w)) * (j + 1)) >> 64              128-bit product, high word: t in [0, j]
 * The multiply-high map is biased by at most (j+1) / 2^64 <= deg / 2^64 per draw.  The cost is O(k) per node whatever
 * its degree; the sample is a pure function of (graph, seeds, fanouts, seed, step).
 *
 * Relabel: local ids 0 .. B-1 are the seeds in the order given (they must be unique: SGX_ERR_SEEDS otherwise, checked on
 * the device).  Hop h samples every node of its frontier (hop 0: the seeds; hop h+1: the nodes that were new at hop h);
 * a sampled node without a local id gets the next one in order of first appearance -- frontier order, then position order
 * within the node's sample.  Outputs:
 *   n_id [nodes]            global id of every local node, seeds first;
 *   out_rowPtr [nodes+1], out_col [edges]
 *                           CSR over local rows: row i holds the sampled neighbours of local node i as local ids, in
 *                           sampled order; rows of the nodes new at the last hop are empty;
 *   edge_pos [edges]        the position in columnIndex (of the input CSR) of every sampled edge, to gather edge values;
 *   hop_nodes [n_hops+1]    HOST: node count before hop 0 (B) and after each hop; hop_edges [n_hops+1] HOST: edge count
 *                           likewise (hop_edges[0] = 0).  nodes = hop_nodes[n_hops], edges = hop_edges[n_hops].
 * node_map [n_nodes] is caller-owned int32 scratch that holds 0x7fffffff (the sentinel) in every entry before the call and
 * again after it (also after SGX_ERR_SEEDS; after any other device-side error the caller refills it).  The relabel uses it
 * instead of a sort: each sampled slot atomicMin's its ordinal into the entry of its node, the slot that finds its own
 * ordinal there is the first appearance, an exclusive scan of those flags gives the new ids, the edges are relabelled
 * through the map and the touched entries reset -- each step its own launch.  One stream synchronisation and one
 * device->host read-back of (2 n_hops + 3) int32 per call; not capturable.
 *
 * Capacity: sgx_sample_workspace_bytes returns the workspace size (0 for bad arguments) and the bounds the outputs are
 * sized from: per hop, edges <= frontier * k (nnz for k == -1), new nodes (the next frontier) <= those edges and <=
 * n_nodes - B; max_edges <= nnz, max_nodes <= n_nodes.  Arguments: n_nodes >= 0, 0 <= nnz < 2^31 - 1, 0 <= batch <= n_nodes, 1 <= n_hops <= 64, fanouts[h] >= -1
 * (fan-outs up to 64 keep the subset in registers, one element per lane; fan-outs of 65 to sgx_sample_wide_max() = 1024
 * keep it in the wavefront's LDS, the whole wavefront at work on the row; only fan-outs over 1024 run a row on one lane
 * in O(k^2) global loads, correct and slow: sgx_sample_form).  max_nodes / max_edges below the bounds: SGX_ERR_SHAPE. */
size_t sgx_sample_workspace_bytes(int n_nodes, int64_t nnz, int batch, int n_hops, const int *fanouts,
                                  int64_t *max_nodes, int64_t *max_edges);
/* Which form of the subset step a hop with this fan-out runs on the rows whose degree exceeds it (rows up to the fan-out
 * are copied whole in every form); the sampler chooses its kernel through this function.  Added without a version bump
 * (SGX_VERSION stays 110): two new declarations, nothing else changes; the same bits come out of every form.
 *   0  fanout == -1: every position, nothing drawn          1  0 .. 64: the subset in registers
 *   2  65 .. sgx_sample_wide_max(): the subset in LDS        3  above: one lane, the subset in the row's output slots
 * fanout < -1: SGX_ERR_SHAPE.  Host queries without a launch and without a device. */
int sgx_sample_wide_max(void);
int sgx_sample_form(int fanout);
int sgx_sample_neighbors(const int32_t *rowPtr, const int32_t *columnIndex, int n_nodes, int64_t nnz,
                         const int32_t *seeds, int batch, int n_hops, const int *fanouts, uint64_t seed, uint64_t step,
                         int32_t *node_map, int32_t *n_id, int32_t *out_rowPtr, int32_t *out_col, int32_t *edge_pos,
                         int64_t max_nodes, int64_t max_edges, int64_t *hop_nodes, int64_t *hop_edges,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- a batch of small graphs through the whole GCN stack in one launch -----------------------
 * The reference's `layer_count` register: how many layers one hardware call processes (demo/<board>/config.py:5,
 * SG.py:1862).  A PyG batch of graphs is sorted: graph g is the row segment [graph_ptr[g], graph_ptr[g+1]) and no edge
 * leaves its graph, so the adjacency is block-diagonal.  One 256-thread workgroup then owns a run of whole graphs and
 * forms every stage for them in LDS -- X.W, aggregation, activation, the next layer, the per-graph mean and the head --
 * without exchanging anything with another workgroup (no flags, no grid barrier; the grid is the plan's group count).
 *
 * Semantics: exactly the chain
 *     sgx_layer_forward(layer 0) -> ... -> sgx_layer_forward(layer n_layers-1) -> sgx_readout_mean_linear
 * (GCN aggregate, SGX_ACC_F32, no plans; every layer as its two stages, sgx_xw_dense / sgx_xw_sparse then sgx_spmm_csr --
 * also the square dense fp16 layer that sgx_layer_forward itself runs with W applied after the aggregation, see
 * sgx_layer_desc.order), with the same rounding points:
 *     H_l = dtype(X_l . W_l)            summed in fp32;  X_0 = the features, X_l = D_{l-1}
 *     D_l = dtype(act_l(A . H_l))       act_l = ReLU where layer[l].relu, else identity
 *     pooled[g][:] = fp32 mean of the rows of graph g of D_{n_layers-1};  logits = bias + W_head . pooled (fp32)
 * and the same summation orders, so every output is bit-equal to that chain:
 *   - aggregation: per row and column an fp32 fma chain over the row's stored entries in CSR order, starting from 0
 *     (the sblock path of sgx_spmm_csr; a row is never split);
 *   - sparse X.W (layer 0, gemm_mode 0): the same fma chain over the feature row's entries (sgx_xw_sparse without a plan,
 *     or with one for every row it does not cut);
 *   - dense X.W: the MFMA shape and K order of sgx_xw_dense (fp16: v_mfma_f32_16x16x32_f16, lane quad q holding k = 32 s
 *     + 8 q .. + 7 of k-step s; fp32: v_mfma_f32_16x16x4_f32, step j of k-block s taking k = 16 s + 4 q + j), k-steps
 *     in ascending order from 0: bit-equal, not merely within an ulp;
 *   - readout: the order of sgx_readout_mean_linear (rows added in order, times 1 / n; the head's lane-strided fmas
 *     over 64 lanes and an xor butterfly, then the bias).
 * Where the plan fits (no graph over its row budget) and every width is within the fused kernel's limits
 * (M_fea, P_w <= the plan's max_width <= 256; a sparse layer 0 may have any M_fea), one launch computes it all.
 * Otherwise sgx_stack_forward runs the chained kernels through the workspace -- same results, so a call always
 * works (single large graphs such as Cora take this path).  GAT layers: `sgx_gat_stack_forward`; quantised layers (GCN or
 * GAT): `sgx_quant_stack_forward`. */
typedef struct sgx_batch_plan sgx_batch_plan;

typedef struct sgx_stack_layer {
    int32_t gemm_mode;    /* layer 0: 0 = CSR features (rowPtr_fea ...), 1 = dense [n_rows][M_fea] in values_fea;
                             layers >= 1 must be 1 (their input is the previous layer's D) */
    int32_t relu;         /* 1: D = max(D, 0) on the rounded value, as sgx_layer_desc.relu */
    int32_t M_fea, P_w;   /* columns of X_l and of D_l; layer l+1 has M_fea = layer l's P_w */
    const void *B;        /* W^T [P_w][M_fea] in dtype, as sgx_layer_desc.B */
    void *D;              /* optional: this layer's output [n_rows][ldd] in dtype (NULL = not written) */
    int64_t ldd;          /* leading dimension of D in elements (0 = P_w) */
} sgx_stack_layer;

typedef struct sgx_stack_desc {
    int32_t dtype, n_layers;                   /* SGX_F16 / SGX_F32; 1 .. 4 */
    int32_t n_rows, n_graphs;                  /* must equal the plan's */
    const int32_t *graph_ptr;                  /* [n_graphs + 1] device, the array the plan was built on */
    const int32_t *rowPtr_adj, *columnIndex_adj; const void *values_adj;   /* [n_rows] x [n_rows] CSR, the plan's */
    const int32_t *rowPtr_fea, *columnIndex_fea; const void *values_fea;   /* layer 0's input */
    sgx_stack_layer layer[4];
    int32_t C;                                 /* head width; 0 = no head (logits not written) */
    const float *W_head, *bias;                /* [C][P_last] fp32, [C] fp32 (bias may be NULL) */
    float *pooled, *logits;                    /* [n_graphs][P_last], [n_graphs][C] fp32; either may be NULL */
    const sgx_batch_plan *plan;                /* from sgx_batch_plan_create */
    void *workspace; size_t workspace_bytes;   /* sgx_stack_workspace_bytes(d), 256-byte aligned (0 on the fused path) */
} sgx_stack_desc;

/* Builds the plan on the device and reads back 16 bytes once (the stream is synchronised; not capturable):
 *   - graph_ptr[0] == 0, monotone, graph_ptr[n_graphs] == n_rows;
 *   - rowPtr_adj monotone, and every stored entry of a row of graph g has its column in graph g;
 * SGX_ERR_BLOCKS when either fails.  Groups are contiguous runs of graphs of at most R rows, R = the LDS row budget for
 * rows of max_width elements of `dtype`, at most 128 (sgx_batch_plan_rows); graph g joins group floor(graph_ptr[g] / S) with
 * S = min(ceil(n_rows / 256), R - largest graph + 1) -- about one group per CU for a small batch, full groups for a large
 * one.  A graph larger than R is recorded (sgx_batch_plan_fits = 0) and the batch then takes the chained path. */
int sgx_batch_plan_create(int dtype, int n_rows, int n_graphs, const int32_t *graph_ptr, const int32_t *rowPtr_adj,
                          const int32_t *columnIndex_adj, int max_width, sgx_batch_plan **plan, void *stream);
int sgx_batch_plan_destroy(sgx_batch_plan *plan);
/* the row budget R, the number of groups, the largest graph's rows, and whether every graph fits (1) or not (0) */
int sgx_batch_plan_rows(const sgx_batch_plan *plan);
int sgx_batch_plan_groups(const sgx_batch_plan *plan);
int sgx_batch_plan_max_graph(const sgx_batch_plan *plan);
int sgx_batch_plan_fits(const sgx_batch_plan *plan);
/* 0 for the fused path, the chained path's scratch otherwise (and for a bad descriptor) */
size_t sgx_stack_workspace_bytes(const sgx_stack_desc *d);
/* Argument errors, returned before anything reaches the device: d, the plan, graph_ptr, the adjacency, layer 0's input,
 * every B, W_head when C > 0: SGX_ERR_NULL; n_layers outside 1..4, n_rows / n_graphs not the plan's, widths that do not
 * chain: SGX_ERR_SHAPE; a dtype other than SGX_F16 / SGX_F32, gemm_mode 0 past layer 0: SGX_ERR_UNSUPPORTED. */
int sgx_stack_forward(const sgx_stack_desc *d, void *stream);

/* ---- training: the backward of that stack in one launch plus one reduction ---------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * Plan kinds: the backward keeps three tiles per row in LDS (X_l / D in dtype, g and G in fp32) where the forward keeps
 * two of dtype, so it needs its own row budget.  sgx_batch_plan_create_ex(..., kind, ...) builds a plan for either
 * kernel; sgx_batch_plan_create is exactly sgx_batch_plan_create_ex(..., SGX_BATCH_FORWARD, ...).  sgx_stack_forward
 * accepts a plan of either kind (its results do not depend on how graphs are grouped), so one SGX_BATCH_BACKWARD plan
 * serves both launches of a training step; sgx_stack_backward takes only SGX_BATCH_BACKWARD plans.
 *
 * Semantics: the backward the layer-by-layer model runs (FPYNQ / RPYNQ / ReadoutMean of sgracex1_amd/molecule_gcn.py:
 * sgx_readout_mean_backward -> per layer sgx_relu_mask_backward, sgx_spmm_csr over the fp32 adjacency, the weight
 * gradient, and sgx_xw_dense(G, W) for the layer below), for the forward of sgx_stack_forward with the same layers:
 *     g_{L-1}[r] = dtype(grad_pooled[graph(r)] * (1 / n_graph))      (sgx_readout_mean_backward's expression)
 *     for l = L-1 .. 0:
 *         g_l[r][c] = 0 where layer[l].relu and D_l[r][c] == 0       (RPYNQ: the mask on the dtype gradient)
 *         G_l    = A . g_l          fp32, per (row, column) an fma chain over the row's stored entries in CSR order from 0
 *                                   (A, not A^T, as the model and the reference multiply)
 *         dW_l   = X_l^T . G_l      fp32 [M_fea][P_w], the layout of the weight parameter; X_0 = the features (CSR or
 *                                   dense), X_l = D_{l-1}
 *         g_{l-1} = dtype(G_l . W_l^T)     (l > 0) W_l the fp32 parameter; the MFMA layout and K order of sgx_xw_dense's
 *                                   fp32 kernel, then one rounding to dtype (autograd's cast to the layer output's type)
 * G_l and every g_l are bit-equal to that chain.  dW_l sums over the batch's rows in another order than the chain's
 * kernels: every workgroup of the launch walks the plan's groups blockIdx.x, blockIdx.x + grid, ... and adds each group's
 * X_l^T . G_l into its own fp32 slice of the workspace (row order within a group, the slice's previous value first;
 * plain loads and stores, no atomics), and a second launch adds the slices in slice order.  The grid is
 * min(max(groups, 1), 512) whatever the device, so a plan gives the same bits on every run and every device; the result
 * stays within the fp32 reordering bound of the chain's X^T . G.
 *
 * Limits: 1 to 4 layers, SGX_F16 / SGX_F32, every P_w and the M_fea of dense layers <= the plan's max_width <= 256 (a
 * sparse layer 0 may have any M_fea; above 16 columns its weight gradient takes a slow path), and a plan that fits.
 * Otherwise SGX_ERR_UNSUPPORTED before anything reaches the device: there is no chained form inside this call (the
 * layer-by-layer autograd path of the model is that form).  Capturable: no allocation and no host synchronisation.
 *
 * Argument errors, returned before anything reaches the device: d, the plan, graph_ptr, the adjacency, layer 0's input,
 * grad_pooled, every W and grad_W, a D the backward reads (D_0 .. D_{L-2}, and D_{L-1} when the last layer has ReLU):
 * SGX_ERR_NULL; n_layers outside 1..4, n_rows / n_graphs not the plan's, widths that do not chain, ldd < P_w:
 * SGX_ERR_SHAPE; a dtype other than SGX_F16 / SGX_F32, gemm_mode 0 past layer 0, a plan of the wrong kind or that does
 * not fit, a width over the limits: SGX_ERR_UNSUPPORTED; workspace missing or smaller than
 * sgx_stack_backward_workspace_bytes: SGX_ERR_WORKSPACE; workspace not 256-byte aligned: SGX_ERR_ALIGN. */
typedef enum sgx_batch_kind {
    SGX_BATCH_FORWARD = 0,          /* row budget of sgx_stack_forward's tiles                   */
    SGX_BATCH_BACKWARD = 1          /* row budget of sgx_stack_backward's (fits both kernels)    */
} sgx_batch_kind;

typedef struct sgx_stack_grad_layer {
    int32_t gemm_mode;    /* as sgx_stack_layer: layer 0 may be 0 (CSR features), layers >= 1 must be 1 */
    int32_t relu;         /* the forward's flag: the gradient is masked where D == 0 */
    int32_t M_fea, P_w;   /* columns of X_l and of D_l */
    const float *W;       /* the fp32 weight parameter [M_fea][P_w] (not transposed) */
    const void *D;        /* the forward's output of this layer [n_rows][ldd] in dtype */
    int64_t ldd;          /* leading dimension of D in elements (0 = P_w) */
    float *grad_W;        /* out: [M_fea][P_w] fp32 */
    float *G;             /* optional out: A . g_l [n_rows][P_w] fp32 (NULL = not written) */
} sgx_stack_grad_layer;

typedef struct sgx_stack_grad_desc {
    int32_t dtype, n_layers;                   /* SGX_F16 / SGX_F32; 1 .. 4 */
    int32_t n_rows, n_graphs;                  /* must equal the plan's */
    const int32_t *graph_ptr;                  /* [n_graphs + 1] device, the array the plan was built on */
    const int32_t *rowPtr_adj, *columnIndex_adj; const void *values_adj;   /* the forward's adjacency (dtype values) */
    const int32_t *rowPtr_fea, *columnIndex_fea; const void *values_fea;   /* layer 0's input, as the forward's */
    sgx_stack_grad_layer layer[4];
    const float *grad_pooled;                  /* [n_graphs][P_last] fp32: the gradient of the pooled means */
    const sgx_batch_plan *plan;                /* from sgx_batch_plan_create_ex(..., SGX_BATCH_BACKWARD, ...) */
    void *workspace; size_t workspace_bytes;   /* sgx_stack_backward_workspace_bytes(d), 256-byte aligned */
} sgx_stack_grad_desc;

int sgx_batch_plan_create_ex(int dtype, int n_rows, int n_graphs, const int32_t *graph_ptr, const int32_t *rowPtr_adj,
                             const int32_t *columnIndex_adj, int max_width, int kind, sgx_batch_plan **plan, void *stream);
/* the weight-gradient slices: min(max(groups, 1), 512) x sum_l M_fea P_w floats; 0 for a descriptor the call refuses */
size_t sgx_stack_backward_workspace_bytes(const sgx_stack_grad_desc *d);
int sgx_stack_backward(const sgx_stack_grad_desc *d, void *stream);

/* ---- shuffled graph mini-batches collated on the device -------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * A graph-classification dataset is uploaded once (sgx_graph_set, device arrays in dataset order) and every mini-batch
 * -- any list of graph ids, such as a slice of a shuffled epoch -- is built from it by one launch of
 * sgx_collate_graphs, exactly as PyG's collation and the CSR builders of the host would build it:
 *   x           the graphs' feature rows, one after another in batch order;
 *   edge_index  int64 [2][n_edges]: each graph's stored edges in stored order plus the graph's first row in the batch;
 *   batch       int64 [n_rows]: the batch position b of every row; y int64 [n_graphs]; graph_ptr int32 [n_graphs+1];
 *   adjacency   the CSR of the edges sorted by (row, col), repeated edges summed, as one block-diagonal matrix: graph
 *               idx[b]'s rows of the dataset's adjacency (whose columns stay inside the graph), columns shifted by
 *               node_off[b] - node_ptr[idx[b]];
 *   features    the CSR of x (zeros dropped): graph idx[b]'s rows of the dataset's, columns unchanged.
 * Values are stored as fp32 and written in each dtype the caller asks for (values_*[SGX_F16] / [SGX_F32], either may be
 * NULL), rounded to nearest even for fp16 -- the same bits as a cast of the fp32 values.
 *
 * The host holds the per-graph counts (rows, stored edges, adjacency and feature entries) and computes the batch's
 * exclusive offsets node_off / edge_off / adj_off / fea_off [n_graphs+1] itself, so the call needs no read-back: one
 * launch (a wavefront per graph), no allocation, no synchronisation; capturable.  Offsets that do not match the set's
 * counts give wrong contents but no write outside the caller's buffers: a graph id outside the set, or a graph whose
 * ranges do not fit the totals, is skipped.
 *
 * Argument errors, returned before anything reaches the device: set, b, any pointer of the set or of the batch that an
 * element is read from or written to (x / edge_index only when there are rows / edges; the values arrays are optional):
 * SGX_ERR_NULL; set->n_graphs < 1, set->n_feat < 1, b->n_graphs < 1, a negative total: SGX_ERR_SHAPE. */
typedef struct sgx_graph_set {
    int32_t n_graphs, n_feat;                  /* graphs of the dataset, feature columns */
    int64_t n_edges;                           /* stored edges of the dataset: the row length of edge_index */
    const int32_t *node_ptr;                   /* [n_graphs+1] first row of every graph */
    const int32_t *edge_ptr;                   /* [n_graphs+1] first stored edge of every graph */
    const int32_t *edge_index;                 /* [2][n_edges] graph-local ids (0 .. rows-1), stored order */
    const float *x;                            /* [rows][n_feat] */
    const int64_t *y;                          /* [n_graphs] */
    const int32_t *rowPtr_adj, *columnIndex_adj; const float *values_adj;   /* block-diagonal adjacency, dataset ids */
    const int32_t *rowPtr_fea, *columnIndex_fea; const float *values_fea;   /* CSR of x */
} sgx_graph_set;

typedef struct sgx_graph_batch {
    int32_t n_graphs, n_rows;                  /* graphs of the batch (>= 1), rows = node_off[n_graphs] */
    int64_t n_edges, nnz_adj, nnz_fea;         /* = edge_off / adj_off / fea_off [n_graphs] */
    const int32_t *index;                      /* [n_graphs] dataset graph id of every batch position */
    const int32_t *node_off, *edge_off, *adj_off, *fea_off;   /* [n_graphs+1] each, exclusive offsets */
    float *x;                                  /* out [n_rows][n_feat] */
    int64_t *edge_index;                       /* out [2][n_edges] */
    int64_t *batch, *y;                        /* out [n_rows], [n_graphs] */
    int32_t *graph_ptr;                        /* out [n_graphs+1] */
    int32_t *rowPtr_adj, *columnIndex_adj;     /* out [n_rows+1], [nnz_adj] */
    void *values_adj[2];                       /* out [nnz_adj] in SGX_F16 / SGX_F32, either may be NULL */
    int32_t *rowPtr_fea, *columnIndex_fea;     /* out [n_rows+1], [nnz_fea] */
    void *values_fea[2];                       /* out [nnz_fea] likewise */
} sgx_graph_batch;

int sgx_collate_graphs(const sgx_graph_set *set, const sgx_graph_batch *b, void *stream);

/* ---- shuffled graph mini-batches with prepared adjacencies ("extras") --------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * Rule.  Let norm_csr(batch) be the adjacency the SGRACE graph classifier builds for a collated batch: sym_norm2 over
 * the batch's edge_index (a self loop of weight fill = 0 for every node without one, unit weights in fp32, the edges
 * sorted by (row, col) with repeated edges kept, value = deg^-1/2[row] * w * deg^-1/2[col] with deg = the row sums)
 * and the row pointer of the sorted rows.  The prepared loader delivers, for every batch, rowPtr / columnIndex /
 * values bit-equal to norm_csr(batch), without computing any of it per batch: it gathers graph idx[b]'s rows of
 * norm_csr(the whole dataset in dataset order) with the columns shifted by node_off[b] - node_ptr[idx[b]].  The two
 * agree because everything in the rule is local to a graph:
 *   - the degree sums add integers (unit weights), so they are exact in fp32 in any order of summation;
 *   - pow(-0.5) and the two multiplications are elementwise, on operands that depend on the graph alone;
 *   - repeated edges stay repeated entries with equal values, in the dataset and in the batch;
 *   - no edge leaves its graph, so the (row, col) sort orders a graph's entries among themselves the same way in the
 *     dataset and in any batch, and a graph's entries are one contiguous range of either.
 * What depends only on a graph's entries can be carried along the same way: the values quantised onto the unsigned
 * adjacency grid (sgx_fake_quantize with signed = 0: csrc/quant_device.h is the one quantiser, run once per dataset
 * and constants) and the dead-row mask (a row with no positive value), of the unquantised and of each quantised
 * value array.
 *
 * sgx_collate_graphs_extras collates the batch exactly as sgx_collate_graphs does and, in the same launch, gathers
 * n_extras (0 .. SGX_COLLATE_MAX_EXTRAS) such dataset-side matrices into the batch.  An extra is a CSR over the
 * dataset's rows (rowPtr / columnIndex in dataset ids, fp32 values, optionally one byte per row) plus the exclusive
 * offsets entry_off [n_graphs+1] of its entries inside the batch, which the host computes from its per-graph entry
 * counts as it does adj_off.  Written per graph: the row pointer (shifted to the batch's entry offsets), the columns
 * (shifted as the adjacency's), the values in each dtype asked for (rounded to nearest even for fp16) and the row
 * bytes, copied.  Several extras may share one pattern (the quantised adjacencies share the normalised one's): an
 * extra with rowPtr_out == NULL and columnIndex_out == NULL writes values and row bytes only, and its rowPtr is read
 * only to find each graph's entry range.
 *
 * The collator's contracts hold: one wavefront per graph, one launch, no allocation, no synchronisation, capturable.
 * A graph id outside the set, or a graph one of whose ranges -- of the batch or of any extra -- does not fit the
 * totals, is skipped as a whole: none of its outputs is written, and nothing is written outside the caller's buffers.
 * n_extras == 0 writes exactly what sgx_collate_graphs writes.
 *
 * Argument errors, returned before anything reaches the device: n_extras outside 0 .. SGX_COLLATE_MAX_EXTRAS:
 * SGX_ERR_SHAPE; then those of sgx_collate_graphs; extras NULL with n_extras > 0, an extra's rowPtr, values or
 * entry_off NULL, columnIndex NULL where the pattern is written, columnIndex_out without rowPtr_out or (with entries)
 * rowPtr_out without columnIndex_out, exactly one of dead_row / dead_row_out NULL (with rows): SGX_ERR_NULL; an
 * extra's nnz < 0: SGX_ERR_SHAPE. */
#define SGX_COLLATE_MAX_EXTRAS 3

typedef struct sgx_collate_extra {
    const int32_t *rowPtr, *columnIndex;       /* dataset side: [rows+1], [entries], dataset ids */
    const float *values;                       /* dataset side: [entries] fp32 */
    const uint8_t *dead_row;                   /* dataset side: [rows], one byte per row; may be NULL */
    int64_t nnz;                               /* entries of the batch = entry_off[n_graphs] */
    const int32_t *entry_off;                  /* device [n_graphs+1], exclusive offsets of every graph's entries */
    int32_t *rowPtr_out, *columnIndex_out;     /* out [n_rows+1], [nnz]; both NULL: the pattern is not written */
    void *values_out[2];                       /* out [nnz] in SGX_F16 / SGX_F32, either may be NULL */
    uint8_t *dead_row_out;                     /* out [n_rows]; NULL exactly when dead_row is */
} sgx_collate_extra;

int sgx_collate_graphs_extras(const sgx_graph_set *set, const sgx_graph_batch *b, const sgx_collate_extra *extras,
                              int n_extras, void *stream);

/* A batch plan from facts the caller already knows (the collator's batches): graph_ptr cuts a block-diagonal adjacency
 * and its largest graph has max_graph rows.  Neither is checked on the device, so nothing is read back:
 * sgx_batch_plan_create_known gives the plan sgx_batch_plan_create_ex gives on the same batch (rows, groups, max_graph,
 * fits and every group_graph entry), computed on the host, with one launch that writes the group_graph table into
 * the caller's device buffer `group_graph` of sgx_batch_plan_group_count(...) + 1 int32 entries.  The plan does not own
 * that buffer (sgx_batch_plan_destroy does not free it), which must outlive the plan's last use.  No allocation, no
 * synchronisation; capturable.  The buffer is not written, and may be NULL, when the plan does not fit or n_graphs == 0.
 * sgx_batch_plan_group_count is host-only: the plan's group count for a batch of n_rows rows in n_graphs >= 1 graphs
 * (0 when the largest graph is over the row budget), or a negative status.
 * Argument errors: plan NULL, graph_ptr NULL with rows or graphs, group_graph NULL where it is written: SGX_ERR_NULL;
 * negative sizes, max_width < 1, max_graph outside [ceil(n_rows / n_graphs), n_rows], rows without graphs: SGX_ERR_SHAPE;
 * a dtype other than SGX_F16 / SGX_F32, an unknown kind: SGX_ERR_UNSUPPORTED. */
int sgx_batch_plan_group_count(int dtype, int n_rows, int max_graph, int max_width, int kind);
int sgx_batch_plan_create_known(int dtype, int n_rows, int n_graphs, const int32_t *graph_ptr, int max_graph, int max_width,
                                int kind, int32_t *group_graph, sgx_batch_plan **plan, void *stream);
/* The plan's group_graph table ([groups + 1] int32: first graph of every group, then n_graphs) copied into dst on the
 * stream (device to device).  Returns the entry count; with dst NULL or capacity below it only the count.  plan NULL:
 * SGX_ERR_NULL. */
int64_t sgx_batch_plan_export_groups(const sgx_batch_plan *plan, int32_t *dst, int64_t capacity, void *stream);

/* ---- padded batches: every full batch of a loader in buffers of one fixed capacity ---------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * A shuffled batch has its own row, edge and entry counts, and those are launch arguments of everything behind the
 * collator, so a recorded step fits one batch.  A PADDED batch has the counts of a capacity the host computes once per
 * (set, B), the spare rows held by well-defined filler graphs; one recorded step then serves every batch of B graphs.
 *
 * Capacity, from the set's per-graph counts:
 *   N         the sum of the B largest row counts (or a row count the caller chooses);
 *   n_min     the sum of the B smallest row counts;  R_f  the largest row count of the set;
 *   F         ceil((N - n_min) / R_f) filler graphs;  G = B + F;
 *   E_cap, fea_cap   the sums of the B largest stored-edge and feature-entry counts;
 *   adj_cap   the sum of the B largest adjacency-entry counts plus N - n_min; an extra's capacity likewise.
 * A batch fits when it has exactly B graphs and its row total n <= N; with the default N every batch of B graphs fits.
 *
 * A padded batch holds its B graphs exactly as sgx_collate_graphs[_extras] writes them, in the live prefix of every
 * array, and behind them P = N - n filler rows in F trailing filler graphs (a the batch's adjacency entries, f its
 * feature entries, E its stored edges):
 *   filler graphs   graph B + k holds clamp(P - k R_f, 0, R_f) rows: graph_ptr[B + k + 1] = n + min(P, (k + 1) R_f);
 *                   the empty ones trail at N (the batch plan's last group takes them, and they pool to 0);
 *                   y[B + k] = 0;
 *   filler row n+j  batch[n + j] = B + j / R_f; its x row is 0; its feature row is empty (rowPtr_fea[n + j] = f); its
 *                   adjacency row holds one diagonal entry of value 1 in each dtype: rowPtr_adj[n + j] = a + j,
 *                   columnIndex_adj[a + j] = n + j, rowPtr_adj[N] = a + P.  The same in every extra, whose row byte is
 *                   0: a GAT row is never dead.  Every filler row's D is 0 in every layer and its gradient is 0;
 *   tails           the entries past the live count up to the capacity are 0, and edge_index[:, E:E_cap] = -1 (the
 *                   padded edge_index is a key, not an edge list, past E).
 * An extra without a pattern of its own (values only: the quantised adjacencies) is refused: SGX_ERR_UNSUPPORTED
 * (sgx_collate_graphs_padded_quant below takes them).
 *
 * sgx_collate_graphs_padded(set, b, extras, n_extras, pad, stream): b->n_graphs = B, and the totals of b and the nnz
 * of the extras are not read -- pad's capacities take their place, as the sizes of the output arrays (graph_ptr
 * [G + 1], y [G]) and as the totals every range is tested against.  The live totals are read on the device from
 * node_off[B], edge_off[B], adj_off[B], fea_off[B] and entry_off[B], so they are no launch arguments.  A graph id
 * outside the set, or a graph whose ranges do not fit the capacities, is skipped as a whole; whatever the offsets
 * hold, nothing is written outside [0, capacity) of any array.  One launch: a wavefront per graph as before, and
 * further workgroups that write the filler rows and the tails with coalesced stores, 16 bytes a lane over the
 * constant ranges.  No allocation, no synchronisation, no atomics; capturable; the same bits on every run.
 *
 * Argument errors: those of sgx_collate_graphs_extras (with the capacities for the totals), pad NULL: SGX_ERR_NULL;
 * G < B, R_f < 0, G R_f < N, a pattern capacity below N - B R_f (what every batch leaves to the fillers) or an entry
 * capacity over INT32_MAX: SGX_ERR_SHAPE. */
typedef struct sgx_collate_pad {
    int32_t n_rows;                            /* N */
    int32_t n_graphs;                          /* G = B + F */
    int32_t filler_rows;                       /* R_f */
    int32_t reserved;
    int64_t n_edges, nnz_adj, nnz_fea;         /* E_cap, adj_cap, fea_cap */
    int64_t nnz_extra[SGX_COLLATE_MAX_EXTRAS]; /* the capacity of every extra */
} sgx_collate_pad;

int sgx_collate_graphs_padded(const sgx_graph_set *set, const sgx_graph_batch *b, const sgx_collate_extra *extras,
                              int n_extras, const sgx_collate_pad *pad, void *stream);

/* Padded batches ready for the QUANTISED layers.  Added without a version bump (SGX_VERSION stays 110): the two
 * declarations below are new, sgx_collate_graphs_padded and everything above it are unchanged (it goes on refusing a
 * values-only extra).
 *
 * sgx_collate_graphs_padded_quant(set, b, extras, n_extras, pad, q, stream) is sgx_collate_graphs_padded -- the same one
 * launch, the same bits in every array that call writes -- with the values-only extras admitted.  An extra k without a
 * pattern of its own (rowPtr_out == columnIndex_out == NULL: a quantised adjacency) shares the pattern of the first
 * pattern-bearing extra met going back from it (the normalised adjacency) and must have that extra's capacity.  Its live entries and
 * row bytes are gathered as sgx_collate_graphs_extras gathers them, so the live prefix holds that call's bits.  Behind
 * them, with a the extra's live entry count, read on the device from its entry_off[B] and clamped to the capacity as
 * every live total is, and fq_k the unsigned-grid device function sgx_fake_quantize(0, qbits[k], inv_scale_adj[k],
 * zero_adj[k]) runs (csrc/quant_device.h, the one quantiser), evaluated in the fill workgroups:
 *   values_out[SGX_F32][a + j] = fq_k(1) for the P = N - n diagonal entries of the filler rows (as far as the capacity
 *                                goes), fq_k(0) from there up to the capacity (values_out[SGX_F16], where given, holds the
 *                                same two numbers rounded to fp16);
 *   dead_row_out[n .. N)       = 0.
 * The call requires, for every values-only extra, fq_k(1) > 0 and fq_k(0) == 0, evaluated on the host by the same
 * function before anything is launched (the check sgx_node_batch_sample_padded_quant makes).  Then a filler graph is as
 * inert under the quantised layers (sgx_quant_stack_forward, sgx_quant_stack_backward) as under the plain ones:
 *   - its feature rows are empty, so X_q . W_q has no term, and the re-quantisation of H (a shift, a clip, a decimal
 *     rounding) leaves a zero row 0;
 *   - its single diagonal entry is live under the mask values_q > 0 and takes softmax weight 1 on a zero H row -- in a GCN
 *     layer the weight fq_k(1) on a zero H row -- so D = 0 after ReLU and deq_factor;
 *   - the next layer reads that D row on its unsigned FEATURE grid (inv_scale_fea, zero_fea of the next layer's
 *     sgx_quant): it stays 0 exactly when that grid maps 0 to 0.  This call does not see those constants; the caller
 *     checks them (pyg_lite.GraphLoader(pad_quant=True) refuses a constant set whose feature grid moves 0) and does not
 *     pad such a set;
 *   - it pools to 0, the loss takes the first B rows of the pooled means, so its grad_pooled row is 0; the backward
 *     forms the same S (weight 1 on the diagonal), every product with its zero rows of X_l, H and g is 0, and no entry
 *     joins it to a live row: its aggregated gradients are 0 and it adds nothing to any weight or attention gradient.
 * A live row may still be dead under the quantised mask alone (an entry may round to 0); the fused attention route
 * declines such a batch, and the loaders do not pad it.
 *
 * The contracts of sgx_collate_graphs_padded stay: one launch of the same shape (a wavefront per graph, fill workgroups
 * with 16-byte stores over the constant ranges), no allocation, no synchronisation, no atomics, plain vector stores,
 * capturable, the same bits on every run, and whatever the offset arrays hold nothing is written outside [0, capacity)
 * of any array.  q is read only for values-only extras (entry k belongs to extras[k]) and may be NULL without one.
 *
 * Argument errors, before anything is launched: n_extras outside 0 .. SGX_COLLATE_MAX_EXTRAS: SGX_ERR_SHAPE; b, pad, or
 * extras with n_extras > 0, NULL: SGX_ERR_NULL; then per values-only extra, in order: q NULL: SGX_ERR_NULL; no
 * pattern-bearing extra before it, or a capacity other than that extra's: SGX_ERR_SHAPE; qbits outside {8, 4, 2, 1}:
 * SGX_ERR_UNSUPPORTED; fq_k(1) <= 0 (or not a number) or fq_k(0) != 0: SGX_ERR_UNSUPPORTED; then everything
 * sgx_collate_graphs_padded returns. */
typedef struct sgx_collate_pad_quant {
    int32_t qbits[SGX_COLLATE_MAX_EXTRAS];         /* 8, 4, 2, 1 */
    float   inv_scale_adj[SGX_COLLATE_MAX_EXTRAS], zero_adj[SGX_COLLATE_MAX_EXTRAS];
} sgx_collate_pad_quant;

int sgx_collate_graphs_padded_quant(const sgx_graph_set *set, const sgx_graph_batch *b, const sgx_collate_extra *extras,
                                    int n_extras, const sgx_collate_pad *pad, const sgx_collate_pad_quant *q, void *stream);

/* The group table of a plan from sgx_batch_plan_create_known written again from `graph_ptr` -- the same n_rows, n_graphs
 * and max_graph, other contents, as a padded batch's buffers hold after the next collation: one launch with the plan's own
 * window and group count into the plan's table.  No allocation, no synchronisation; capturable.  A plan without a table
 * (it does not fit) is left alone.  plan NULL, graph_ptr NULL: SGX_ERR_NULL; a plan that owns its table (its batch was
 * checked on the device, and another is not): SGX_ERR_UNSUPPORTED. */
int sgx_batch_plan_regroup(const sgx_batch_plan *plan, const int32_t *graph_ptr, void *stream);

/* ---- layer-ready node batches: a neighbour sample prepared on the device ----------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_node_batch_sample runs sgx_sample_neighbors (same arguments, same results) and, behind it on the same stream
 * without reading anything back in between, builds what the SGRACE layers need from the sample (csrc/node_batch.hip).
 * The counts the host needs ride the sampler's one read-back, which stays the only one of the call.
 *
 * Normalised adjacency -- sym_norm2 (SG.py:18-51) of the sampled CSR, in the orientation the layers aggregate in (row i =
 * the neighbours sampled for local node i), as the CSR the layer reads; n = nodes rows and columns:
 *   - entry weights w: edge_weight[edge_pos[e]] (edge_weight indexed like columnIndex of the input graph), or 1 when
 *     edge_weight is NULL;
 *   - every row without a stored self loop gets one of weight `fill`; stored loops keep their weight;
 *   - the entries of a row are ordered by column, stably: repeated edges stay separate entries in sampled order, and the
 *     added loop comes after stored entries of its column (there are none, or it would not be added -- the rule fixes
 *     the order for the restatement all the same);
 *   - deg[r] = the row's weights added one by one in that stored order, in fp32, starting from 0;
 *   - dis[r] = deg[r] > 0 ? 1 / sqrt(deg[r]) : 0, the square root and then the division each the IEEE-754 correctly
 *     rounded fp32 operation;
 *   - value = (dis[r] * w) * dis[c]: the left product rounded to fp32, then the right one, then one rounding to `dtype`
 *     (SGX_F32: none).
 * The result is a pure function of the sample, edge_weight and fill: the same bits on every run.
 *   rowPtr_norm [nodes+1] = out_rowPtr + the exclusive count of rows that got a loop; columnIndex_norm, values_norm
 *   [nnz_norm <= edges + nodes]; dead_row [nodes] bytes: 1 where the row holds no stored value > 0 (after the rounding
 *   to dtype) -- the rows the GAT mask `adj > 0` leaves without a neighbour.
 *   edge_index_agg / edge_index: int64 [2][edges], written at [0, edges) and [edges, 2 edges) of buffers of 2 max_edges
 *   entries: row 0 the aggregating node and row 1 its sampled neighbour / PyG's orientation, the two rows swapped.
 *   Either may be NULL.
 * Features (optional, rowPtr_x != NULL): the CSR (rowPtr_x, columnIndex_x, values_x fp32) of the whole graph's feature
 * matrix; rows n_id of it, in that order, are copied to rowPtr_fea [nodes+1], columnIndex_fea, values_fea (in dtype, the
 * fp32 value rounded to nearest even) -- the CSR a dense-to-CSR conversion of the gathered rows gives.  fea_capacity =
 * the entries columnIndex_fea / values_fea hold; a batch that needs more fails with SGX_ERR_SHAPE, nothing written
 * outside.  Labels (optional): y_out[i] = y[n_id[i]] (int64), mask_out[m][i] = mask[m][n_id[i]] (bytes), each NULL or
 * given.
 * Host results: hop_nodes / hop_edges as sgx_sample_neighbors; nnz_norm, nnz_fea, has_dead_rows (some dead_row is 1),
 * max_row (the longest row of the normalised matrix).
 *
 * Capacity: sgx_node_batch_workspace_bytes is sgx_sample_workspace_bytes for this call (same bounds max_nodes /
 * max_edges; more bytes).  rowPtr_norm holds max_nodes + 1 entries, columnIndex_norm / values_norm max_edges + max_nodes,
 * dead_row / y_out / mask_out max_nodes, rowPtr_fea max_nodes + 1.  Nothing allocates.  Status codes and the node_map
 * contract are the sampler's; dtype other than SGX_F16 / SGX_F32: SGX_ERR_UNSUPPORTED.  batch == 0: the three row
 * pointers get their single 0 and the call returns without a read-back.  Not capturable. */
typedef struct sgx_node_batch {
    /* the sampler's arguments (sgx_sample_neighbors) */
    const int32_t *rowPtr, *columnIndex;
    int32_t n_nodes, batch, n_hops, dtype;     /* dtype: element type of values_norm and values_fea */
    int64_t nnz;
    const int32_t *seeds;
    const int *fanouts;                        /* HOST [n_hops] */
    uint64_t seed, step;
    int32_t *node_map, *n_id, *out_rowPtr, *out_col, *edge_pos;
    int64_t max_nodes, max_edges;
    int64_t *hop_nodes, *hop_edges;            /* HOST out [n_hops+1] each */
    /* normalised adjacency */
    const float *edge_weight;                  /* [nnz] or NULL */
    float fill;
    int32_t *rowPtr_norm, *columnIndex_norm;
    void *values_norm;
    uint8_t *dead_row;
    int64_t *edge_index, *edge_index_agg;
    /* features and labels */
    const int32_t *rowPtr_x, *columnIndex_x;
    const float *values_x;
    int32_t *rowPtr_fea, *columnIndex_fea;
    void *values_fea;
    int64_t fea_capacity;
    const int64_t *y;
    int64_t *y_out;
    const uint8_t *mask[3];
    uint8_t *mask_out[3];
    /* host results */
    int64_t nnz_norm, nnz_fea;
    int32_t has_dead_rows, max_row;
    void *workspace;
    size_t workspace_bytes;
} sgx_node_batch;

size_t sgx_node_batch_workspace_bytes(int n_nodes, int64_t nnz, int batch, int n_hops, const int *fanouts,
                                      int64_t *max_nodes, int64_t *max_edges);
int sgx_node_batch_sample(sgx_node_batch *b, void *stream);

/* Layer-ready for the QUANTISED layers.  Added without a version bump (SGX_VERSION stays 110): the two declarations below
 * are new, sgx_node_batch and everything above it are unchanged.
 *
 * sgx_node_batch_sample_quant(b, q) is sgx_node_batch_sample(b) -- same arguments, same results, bit for bit -- and, on the
 * same stream before the call's one read-back, for each of the q->n_sets constant sets k (the adjacency constants of the
 * layers that will read the batch: layer 1 / layer 2 of the demo) also writes what the quantised layers otherwise build
 * per batch from values_norm:
 *   values_q[k][e]   = the unsigned-grid value sgx_fake_quantize(0, qbits, inv_scale_adj[k], zero_adj[k]) gives for
 *                      values_norm[e], e < nnz_norm: computed by the device function that call runs (csrc/quant_device.h),
 *                      so the bits equal a sgx_fake_quantize launch over values_norm;
 *   dead_row_q[k][r] = 1 where row r holds no values_q[k] > 0: the rows the GAT mask leaves without a neighbour once the
 *                      adjacency is quantised (an entry may round to 0, so a row live in values_norm may be dead here);
 *   values_lean[k][e] (optional, NULL = not written) = values_norm[e] on the rows with dead_row_q[k], values_q[k][e]
 *                      elsewhere: the one values array the statistics form of the GAT backward masks with;
 *   has_dead_rows_q[k] (host) = some dead_row_q[k] is 1.  It rides the sampler's counter block, so the call still has
 *                      exactly one device-to-host copy.
 * values_q / values_lean hold max_edges + max_nodes fp32 entries, dead_row_q max_nodes bytes.  Nothing allocates; no
 * workspace beyond sgx_node_batch_workspace_bytes.  Two sets may carry equal constants; both are then written.
 * Argument errors, returned before anything is launched and with the node_map untouched: b or q NULL: SGX_ERR_NULL;
 * b->dtype other than SGX_F32 (the quantised layer works on fp32): SGX_ERR_UNSUPPORTED; n_sets outside {1, 2} or qbits
 * outside {8, 4, 2, 1}: SGX_ERR_SHAPE; values_q[k] or dead_row_q[k] NULL for a k < n_sets: SGX_ERR_NULL; then those of
 * sgx_node_batch_sample.  batch == 0 returns as sgx_node_batch_sample does, has_dead_rows_q = 0.  Not capturable. */
typedef struct sgx_node_batch_quant {
    int32_t n_sets;                 /* 1 or 2 constant sets (layer 1 / layer 2) */
    int32_t qbits;                  /* 8, 4, 2, 1 */
    float   inv_scale_adj[2], zero_adj[2];
    float  *values_q[2];            /* out [max_edges + max_nodes] fp32 */
    uint8_t *dead_row_q[2];         /* out [max_nodes] */
    float  *values_lean[2];         /* out, optional (NULL = not written) */
    int32_t has_dead_rows_q[2];     /* HOST out */
} sgx_node_batch_quant;
int sgx_node_batch_sample_quant(sgx_node_batch *b, sgx_node_batch_quant *q, void *stream);

/* ---- the layer's backward in one call ---------------------------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_layer_backward is the backward of sgx_layer_forward for the SGRACE layer (FPYNQ_GAT.backward, SG.py:884-1126, the
 * `accb == 0` formulas on the stored entries), all in fp32, with P and not P^T as the reference multiplies:
 *     GAT:  Wh = X . W                                       sgx_xw_dense (after sgx_transpose of W) / sgx_xw_sparse
 *           sg, g1 = the edge pass                            sgx_gat_backward_edges (E, S) or ..._edges_stats (stats)
 *           grad_attention = [ Wh^T g1 ; Wh^T colsum(sg) ]    sgx_gat_attention_grad
 *           P = S on the stored entries; a dead row = 1/N on every column
 *     GCN:  P = the adjacency values as fp32 (SGX_F16 values are cast into the workspace); grad_attention is not written
 *     both: pg = P . G                                        sgx_spmm_csr; rows with dead[r]: colsum(G) * (1/N)
 *           grad_input   = pg . W^T                           sgx_xw_dense(pg, Wt := W); not launched when grad_input is NULL
 *           grad_weights = X^T . pg                           sgx_xt_g, or sgx_spmm_csr over the CSR of X^T (gemm_mode 0)
 * 1/N is the fp32 reciprocal of N_adj, rounded once, and multiplies the fp32 column sums (sgx_col_sums); the softmax
 * row sum the edge pass takes for a dead row is G[r] . (colsum(Wh) * (1/N)) through sgx_xw_dense.  Every product runs on
 * the stage kernel named, so grad_input and grad_weights carry the bits those calls give on the same operands.
 *
 * The forward's state is given in ONE of two forms: E and S (both), or stats with dead_weight (the S of a dead row's
 * stored entries, 1/N for the layer).  Neither, or only one of E / S: SGX_ERR_NULL; E / S and stats together:
 * SGX_ERR_UNSUPPORTED.  values_adj is the array the edge-pass call of the form takes as `values`: the mask `adj > 0` is
 * read from it.  dead (optional, bytes [N_adj]): the rows the forward found without a positive entry.
 *
 * Argument errors, returned before anything reaches the device: d or a required pointer NULL: SGX_ERR_NULL; a size
 * below 1, N_adj != M_adj (P . G needs a square P), ldg < P_w, ldx < M_fea, ld_gi < M_fea: SGX_ERR_SHAPE; gat_heads > 1,
 * a mode outside {0, 1}, a dtype other than SGX_F16 / SGX_F32, tables past 32-bit byte offsets: SGX_ERR_UNSUPPORTED;
 * workspace missing or below sgx_layer_backward_workspace_bytes: SGX_ERR_WORKSPACE; not 256-byte aligned: SGX_ERR_ALIGN.
 * Asynchronous on `stream`, no allocation, no synchronisation: capturable. */
typedef struct sgx_layer_grad_desc {
    int32_t gat_mode;    /* 0: GCN, 1: single-head GAT                                             */
    int32_t gemm_mode;   /* 0: X as CSR (and the CSR of X^T), 1: X dense                           */
    int32_t N_adj;       /* rows of the adjacency, of G and of grad_input                          */
    int32_t M_adj;       /* columns of the adjacency = rows of X; must equal N_adj                 */
    int32_t M_fea;       /* columns of X = rows of W                                               */
    int32_t P_w;         /* columns of W and of G                                                  */
    int32_t dtype_adj;   /* sgx_dtype of values_adj                                                */
    int32_t dtype_x;     /* sgx_dtype of the dense X (gemm_mode 1); CSR feature values are fp32    */
    int32_t gat_heads;   /* 0 or 1; more: SGX_ERR_UNSUPPORTED                                      */
    float   alpha;       /* LeakyReLU slope                                                        */
    int64_t nnz_adj;     /* stored entries of the adjacency (sizes the per-entry scratch)          */

    const int32_t *rowPtr_adj;        /* [N_adj+1]                                                 */
    const int32_t *columnIndex_adj;   /* [nnz_adj]                                                 */
    const void    *values_adj;        /* [nnz_adj] in dtype_adj                                    */
    const sgx_plan *plan_adj;         /* optional: the schedule of P . G                           */

    const void    *X;                 /* gemm_mode 1: [M_adj][ldx] in dtype_x                      */
    int64_t        ldx;
    const int32_t *rowPtr_fea;        /* gemm_mode 0, GAT: the CSR of X, fp32 values (Wh = X . W)  */
    const int32_t *columnIndex_fea;
    const float   *values_fea;
    const sgx_plan *plan_fea;         /* optional                                                  */
    const int32_t *rowPtr_xt;         /* gemm_mode 0: the CSR of X^T [M_fea] x [M_adj], fp32       */
    const int32_t *columnIndex_xt;
    const float   *values_xt;
    const sgx_plan *plan_xt;          /* optional                                                  */

    const float   *W;                 /* the fp32 weight parameter [M_fea][P_w] (not transposed)   */
    const float   *G;                 /* grad_output [N_adj][ldg] fp32                             */
    int64_t        ldg;
    const float   *E;                 /* GAT, form 1: the forward's per-entry outputs [nnz_adj]    */
    const float   *S;
    const sgx_gat_stats *stats;       /* GAT, form 2: the forward's row statistics                 */
    float          dead_weight;       /* form 2: S on the stored entries of a dead row             */
    const uint8_t *dead;              /* optional [N_adj]: 1 = the forward's dead rows             */

    float         *grad_weights;      /* out [M_fea][P_w]                                          */
    float         *grad_attention;    /* out [2 P_w], GAT only                                     */
    float         *grad_input;        /* out [N_adj][ld_gi], pad columns zeroed; NULL = not formed */
    int64_t        ld_gi;

    void          *workspace;         /* sgx_layer_backward_workspace_bytes(d), 256-byte aligned   */
    size_t         workspace_bytes;

    /* Appended without a version bump (SGX_VERSION stays 110): all five are 0 in a descriptor that was zeroed, and 0 is
     * the call as it was -- the same workspace size, status and bits.
     * schedule_adj / schedule_fea / schedule_xt: sgx_layer_schedule_kind, per matrix.  Under SGX_SCHEDULE_FLAT the
     * products over that matrix run on the entry-split schedule ("entry-split aggregation" above): no plan, nothing read
     * back, every grid a function of the descriptor's host fields, so the call records into a graph and replays on other
     * matrices inside the same capacities, whatever their rows are like.
     *   schedule_adj   pg = P . G runs as sgx_spmm_csr_flat at nnz_adj and (GAT) the attention gradient as
     *                  sgx_gat_attention_grad_flat at nnz_adj.  The edge pass and the dead-row select stay as they are:
     *                  the edge pass reads its entry count from rowPtr_adj[N_adj] on the device, touches nothing at or
     *                  behind it and sizes its launches by N_adj and the device alone.  nnz_adj is then a capacity: the
     *                  entries columnIndex_adj / values_adj (and E, S) hold, a bound on rowPtr_adj[N_adj].
     *   schedule_fea   GAT, gemm_mode 0: Wh = X . W runs as sgx_spmm_csr_flat(fea, W) at nnz_fea.  Not read otherwise.
     *   schedule_xt    gemm_mode 0: grad_weights runs as sgx_spmm_csr_flat(X^T, pg) at nnz_xt.  Not read in gemm_mode 1.
     * nnz_fea / nnz_xt: the entries columnIndex_fea / _xt and values_fea / _xt hold; read only under their flat schedule.
     * THE RULE is the one above: every output equals the named stage calls composed on the same operands and capacities,
     * bit for bit -- the edge pass, then the flat calls, then sgx_xw_dense / sgx_xt_g.
     * The scratch of the flat calls lies behind the default layout inside `workspace`, each on a 256-byte boundary
     * (sgx_layer_backward_workspace_bytes accounts for it at the capacities).
     * Refused before any launch: a schedule that is read and is neither enumerator, or SGX_SCHEDULE_FLAT together with the
     * plan of the same matrix (plan_adj / plan_fea / plan_xt): SGX_ERR_UNSUPPORTED; a capacity that is read and lies outside
     * [0, INT32_MAX]: SGX_ERR_SHAPE (INT32_MAX itself is a capacity like any other, as in the entry-split calls; under the
     * default schedule nnz_adj = INT32_MAX stays SGX_ERR_UNSUPPORTED);
     * a table a flat product gathers (G, W, pg) past 32-bit byte offsets: SGX_ERR_UNSUPPORTED. */
    int32_t        schedule_adj, schedule_fea, schedule_xt;
    int64_t        nnz_fea, nnz_xt;
} sgx_layer_grad_desc;

/* 0 for a descriptor the call refuses (workspace and workspace_bytes are not looked at) */
size_t sgx_layer_backward_workspace_bytes(const sgx_layer_grad_desc *d);
int    sgx_layer_backward(const sgx_layer_grad_desc *d, void *stream);
/* Which schedules sgx_layer_backward takes for this descriptor, for reports and tests (a new declaration, no version
 * bump): a host query without a launch that reads no device memory and neither workspace field, answered by the checks
 * the call itself makes.  Bit 0: the adjacency's products, bit 1: Wh = X . W, bit 2: grad_weights = X^T . pg run
 * entry-split (a schedule field that is not read leaves its bit 0); negative: the sgx_status the call would return. */
int    sgx_layer_backward_schedule(const sgx_layer_grad_desc *d);

/* The attention gradient of the GAT backward from the edge pass's outputs, without a transposed pattern:
 *     grad_attention[0:F]  = Wh^T g1            = sum_r g1[r] Wh[r]
 *     grad_attention[F:2F] = Wh^T colsum(sg)    = sum_r t_r,   t_r[f] = sum_{e in row r} sg_e Wh[col_e][f]
 * t_r is an fp32 fma chain over the row's stored entries in CSR order from 0; a row over 256 entries is cut into chunks
 * of 256 entries, each such a chain, whose sums are added in chunk order.  Rows of Wh are gathered through a range-checked
 * buffer, 16 bytes per lane when Wh is 16-byte aligned and ldw a multiple of 4, one element at a time otherwise.
 * Grid rule: slices = min(max(ceil(n_rows / 64), 1), 1024) workgroups of 256 threads whatever the device; workgroup b owns
 * rows [b R, (b+1) R), R = ceil(n_rows / slices).  Its 4 * 64 / L lane groups (L = the power of two >= ceil(F / 4), at most
 * 64) take rows b R + k, b R + k + 256 / L, ... in ascending order and add g1[r] Wh[r] and t_r into registers; the groups'
 * sums are added in group order, then the rows over 256 entries in ascending order, and stored to the workgroup's slice
 * (plain loads and stores, no atomics); a second launch adds the slices in slice order.  The same bits on every run and
 * every device.  n_rows <= n_cols (row r of the adjacency is node r of Wh).  workspace:
 * sgx_gat_attention_grad_workspace_bytes(n_rows, F) bytes (slices x 2 F floats), 256-byte aligned.  n_rows == 0, or a
 * matrix without entries and g1 = 0: both halves are exactly 0. */
size_t sgx_gat_attention_grad_workspace_bytes(int n_rows, int n_feat);
int sgx_gat_attention_grad(int n_rows, int n_cols, int n_feat, const int32_t *rowPtr, const int32_t *columnIndex,
                           const float *sg, const float *g1, const float *Wh, int64_t ldw, float *grad_attention,
                           void *workspace, size_t workspace_bytes, void *stream);

/* The same two outputs by stored entries (added without a version bump: new declarations).  Neither half has rows --
 * grad_attention[F:2F] = sum_{e < end} sg_e Wh[col_e] is one reduction over all stored entries -- so the schedule is a
 * function of nnz, n_rows, F and Wh's alignment alone, balanced on any degree distribution: a hub row is spread over the
 * chunks its entries fall in instead of being walked by one workgroup.  The rule, with T = sgx_spmm_flat_chunk():
 *   - end = min(rowPtr[n_rows], nnz), read on the device.  nnz is a host argument and may be a capacity: a bound on
 *     rowPtr[n_rows], and no more than columnIndex / sg hold.  Nothing at or behind end, and nothing behind the capacity,
 *     is read, whatever rowPtr holds.
 *   - the entries are cut into chunks of T consecutive entries, chunk c = [cT, min((c+1)T, end)), and the rows into
 *     chunks of T consecutive rows for the first half; one wavefront per chunk.  No search in rowPtr is made.
 *   - inside a chunk, L lanes (L = the power of two >= ceil(F / 4), at most 64; 16 bytes of a Wh row each) form a lane
 *     group, 64 / L groups; group g takes items g, g + 64 / L, ... of the chunk in ascending order: one fp32 fma per item
 *     and column, sg_e Wh[col_e][f] (g1[r] Wh[r][f] for a row chunk) onto a register that starts at +0.  The groups' sums
 *     are added in group order, group 0 first, and the chunk's partial row [F] is stored to the workspace.
 *   - a second launch adds the partials of a half by chunk index in a fixed two-level order: chain q = 0 .. 15 adds the
 *     chunks q, q + 16, q + 32, ... below ceil(end / T) (ceil(n_rows / T) for the first half) in ascending order from +0;
 *     the 16 chains are added in order q from +0 and the element is stored once.
 * Rows of Wh are gathered through a range-checked buffer, 16 bytes per lane when Wh is 16-byte aligned and ldw a multiple
 * of 4, one element at a time otherwise (the same sums).  Plain loads and stores, no atomics, every output element written
 * once; chunks at or past end write nothing and the second launch does not read them: the result has the same bits on
 * every run and for every capacity nnz >= rowPtr[n_rows].  n_rows == 0, or end == 0 with g1 = 0: both halves exactly +0.
 * The longest addition chain of an element: T L / 64 + 64 / L + ceil(chunks / 16) + 16.
 * workspace: sgx_gat_attention_grad_flat_workspace_bytes(nnz, n_rows, F) bytes (0 for nnz outside [0, INT32_MAX],
 * n_rows < 0 or F < 1), 256-byte aligned.  Argument errors are those of sgx_gat_attention_grad, and nnz outside
 * [0, INT32_MAX]: SGX_ERR_SHAPE; all are returned before anything reaches the device.  Asynchronous on `stream`, no
 * allocation, no synchronisation: capturable, and a recorded call replays on any matrix inside the capacity. */
size_t sgx_gat_attention_grad_flat_workspace_bytes(int64_t nnz, int n_rows, int n_feat);
int    sgx_gat_attention_grad_flat(int n_rows, int n_cols, int n_feat, int64_t nnz,
                                   const int32_t *rowPtr, const int32_t *columnIndex,
                                   const float *sg, const float *g1, const float *Wh, int64_t ldw,
                                   float *grad_attention, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the transpose of a CSR matrix -------------------------------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_csr_transpose writes the CSR of A^T ([n_cols] rows, [n_rows] columns) for a CSR A of n_rows x n_cols with nnz stored
 * entries: rowPtr_t [n_cols + 1], columnIndex_t [nnz], values_t [nnz], and optionally order [nnz].  Rule:
 *     entry k of A^T is stored entry order[k] of A;  columnIndex_t[k] = the row of A that holds entry order[k];
 *     values_t[k] = values[order[k]], copied bit for bit (-0.0, NaN payloads and subnormals survive);
 *     within a row of A^T the entries stand in ascending order[k]: the transpose is STABLE.
 * Where every (row, col) pair of A is stored once that is the order by (col, row); copies of a pair keep their source
 * order.  order = the stable sort of the positions 0 .. nnz-1 by columnIndex; rowPtr_t[c] = the number of stored entries
 * with a column below c.  The result is a pure function of the input: the same bits on every run, every device and every
 * grid size (a least-significant-digit radix sort, 8 bits a pass, ceil(bits(n_cols - 1) / 8) passes over tiles of
 * SGX_CSR_TRANSPOSE_TILE entries; integer atomics only count, no output position depends on the order in which one
 * returns).  The work is O(nnz x passes + n_cols log nnz) whatever the lengths of the rows of A^T.
 *
 * values and values_t are both NULL (a pattern only; dtype_values is then not looked at) or both given (dtype_values:
 * SGX_F16 or SGX_F32).  order may be NULL.  The input arrays are not modified; no output may alias an input or another
 * output.  Index and order arrays need 4-byte alignment only, fp16 values 2-byte (slices of larger buffers are fine).
 * workspace: sgx_csr_transpose_workspace_bytes(n_rows, n_cols, nnz) bytes, 256-byte aligned.  The contents of an invalid
 * CSR are the caller's to check (sgx_csr_validate); whatever they are, nothing is read or written out of bounds.
 * n_rows == 0 or nnz == 0: rowPtr_t becomes all zeros and nothing else is written.
 *
 * Argument errors, returned before anything reaches the device: rowPtr, columnIndex, rowPtr_t or columnIndex_t NULL, or
 * exactly one of values / values_t NULL: SGX_ERR_NULL; n_rows, n_cols or nnz below 0: SGX_ERR_SHAPE; nnz > INT32_MAX, or
 * (with values) a dtype other than SGX_F16 / SGX_F32: SGX_ERR_UNSUPPORTED; workspace missing or too small:
 * SGX_ERR_WORKSPACE; not 256-byte aligned: SGX_ERR_ALIGN.  Asynchronous on `stream`, no allocation, no synchronisation:
 * capturable. */
#define SGX_CSR_TRANSPOSE_TILE 2048   /* stored entries per workgroup of a sort pass */

/* 0 for sizes the call refuses; otherwise positive and a multiple of 256 */
size_t sgx_csr_transpose_workspace_bytes(int n_rows, int n_cols, int64_t nnz);
int sgx_csr_transpose(int dtype_values, int n_rows, int n_cols, int64_t nnz,
                      const int32_t *rowPtr, const int32_t *columnIndex, const void *values,
                      int32_t *rowPtr_t, int32_t *columnIndex_t, void *values_t, int32_t *order,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- GAT layers in the small-graph stack ------------------------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_gat_stack_forward is sgx_stack_forward with a per-layer choice of the aggregate: the reference's `layer_count`
 * register sits on the same bitstream as `gat_mode` (SG.py:1862).  It takes the same sgx_batch_plan, of either kind --
 * the row budget and the grouping of plans are those of sgx_stack_forward, so one plan (cached on a batch) serves the
 * GCN and the GAT calls -- and runs the same one launch: a 256-thread workgroup per group of whole graphs, every stage
 * in LDS, nothing exchanged between workgroups (no flags, no grid barrier; the grid is the plan's group count).
 *
 * Semantics, per layer l:
 *     H_l = dtype(X_l . W_l)            exactly as in sgx_stack_forward: the sparse layer 0 by the fma chain in CSR order,
 *                                       dense layers in the MFMA layout and K order of sgx_xw_dense -- bit-equal to them
 *   gat_mode = 0:
 *     D_l = dtype(act_l(A . H_l))       the GCN layer of sgx_stack_forward, bit for bit
 *   gat_mode = 1: sgx_gat_aggregate's single-head formula on H_l as stored, attention = [a1 ; a2], [2 * P_w] in dtype:
 *     s1_i = H_i . a1,  s2_c = H_c . a2                                  in fp32
 *     x_e  = LeakyReLU_alpha(s1_i + s2_c)                                on stored entries e = (i, c) with values[e] > 0, the
 *                                                                        stored value as stored (+0.0, -0.0 and negative
 *                                                                        values are masked, positive subnormals are live)
 *     m_i  = max over the row's live entries;  S_e = exp(x_e - m_i) / sum_live exp(x - m_i)
 *     D_i  = dtype(act_l(sum_e S_e H_c))                                 summed in fp32
 *     a row without a live entry gives 0 (the gat_fill_dead_rows = 0 rule; the mean-of-all-rows rule reaches across the
 *     batch's graphs and is not offered).  E, S and the row statistics are not outputs: this is the inference path.
 *     One head only.
 *   readout and head: as in sgx_stack_forward, the same bits for the same D_{n_layers-1}.
 * Summation order of the attention path is not pinned: its results lie inside the bound of tests/_gat_ref.py (whose
 * docstring derives it; the exponential is the hardware's v_exp_f32 on (x - m) log2(e), the division one reciprocal of
 * the sum and a product) and are the same bits on every run, on every device and for every grouping of the graphs: no
 * atomics, and no order that depends on the grid -- a row's sums are split over lanes by the layer's width alone.
 *
 * Where the plan fits and every width is within the fused kernel's limits (those of sgx_stack_forward), one launch
 * computes it all; sgx_gat_stack_workspace_bytes is 0 exactly then.  The four fp32 arrays s1, s2, m, 1 / sum of a group's
 * rows lie in LDS behind the two tiles (16 bytes per row of the budget, at most 2 KiB; where the tiles fill 64 KiB --
 * fp32 at width 252 -- the launch asks for that much more, still two workgroups per CU).  Otherwise the call runs the
 * chained kernels through the workspace: per layer X.W as in sgx_stack_forward's chain, then
 * sgx_gat_aggregate(fill_dead_rows = 0, one head, no plan) or the GCN aggregate, then sgx_readout_mean_linear -- inside
 * the same bound, so a call always works.
 *
 * Argument errors, returned before anything reaches the device: those of sgx_stack_forward, and attention NULL on a layer
 * with gat_mode = 1: SGX_ERR_NULL; gat_mode outside {0, 1}: SGX_ERR_UNSUPPORTED.  Capturable on the fused path: no
 * allocation and no host synchronisation. */
typedef struct sgx_gat_stack_layer {
    int32_t gemm_mode;    /* as sgx_stack_layer */
    int32_t relu;
    int32_t M_fea, P_w;
    const void *B;
    void *D;
    int64_t ldd;
    int32_t gat_mode;     /* 0: GCN aggregate (A . H); 1: the edge softmax above */
    const void *attention;   /* gat_mode = 1: [2 * P_w] in dtype, a1 then a2, as sgx_layer_desc.attention */
    float alpha;          /* LeakyReLU slope of the scores */
} sgx_gat_stack_layer;

typedef struct sgx_gat_stack_desc {
    int32_t dtype, n_layers;                   /* as sgx_stack_desc, field for field */
    int32_t n_rows, n_graphs;
    const int32_t *graph_ptr;
    const int32_t *rowPtr_adj, *columnIndex_adj; const void *values_adj;
    const int32_t *rowPtr_fea, *columnIndex_fea; const void *values_fea;
    sgx_gat_stack_layer layer[4];
    int32_t C;
    const float *W_head, *bias;
    float *pooled, *logits;
    const sgx_batch_plan *plan;                /* from sgx_batch_plan_create / _create_ex / _create_known, either kind */
    void *workspace; size_t workspace_bytes;   /* sgx_gat_stack_workspace_bytes(d), 256-byte aligned (0 on the fused path) */
} sgx_gat_stack_desc;

/* 0 for the fused path, the chained path's scratch otherwise (and for a bad descriptor) */
size_t sgx_gat_stack_workspace_bytes(const sgx_gat_stack_desc *d);
int sgx_gat_stack_forward(const sgx_gat_stack_desc *d, void *stream);

/* A plain streaming copy (16 bytes per lane, non-temporal, each workgroup on a contiguous chunk), the kernel the attainable HBM rate of a device is
 * measured with next to the nominal 8 TB/s (bench.py reports it as roofline.stream_copy_GBps_this_device).
 * bytes must be a multiple of 16, both pointers 16-byte aligned. */
int sgx_stream_copy(void *dst, const void *src, int64_t bytes, void *stream);

/* hipEvent_t helpers for the profiling taps of sgx_layer_desc (handles travel as void*), so that
 * a host that does not link the HIP runtime itself can time launches on the library's runtime.
 * sgx_event_elapsed_ms waits for `end` and returns the milliseconds between the two events. */
int sgx_event_create(void **event);
int sgx_event_destroy(void *event);
int sgx_event_record(void *event, void *stream);
int sgx_event_elapsed_ms(void *begin, void *end, float *ms);

int         sgx_version(void);
const char *sgx_status_string(int status);

/* The library reads its SGX_* tuning overrides from the environment once, at its first use.  A process that changes one
 * of them later (a test comparing two kernel forms) calls this to have them read again.  Not for concurrent use with
 * other calls into the library. */
void sgx_reload_env(void);

/* ---- quantised layers in the small-graph stack -------------------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_quant_stack_forward is sgx_gat_stack_forward with a per-layer quantiser: the reference's `layer_count` register
 * belongs to the quantised bitstream (gat_all_unsigned.bit), whose every board config ships with the quantiser on.  It
 * takes the same sgx_batch_plan, of either kind, so one plan cached on a batch serves all three stack calls, and on the
 * fused path it is the same one launch: the quantisers sit on the operand loads and the two stores of the stages.
 * Parity of the quantised layer is UNPINNED, here as everywhere: the reference records no quantised output; what is
 * pinned is equality with this library's own sgx_layer_forward (tests/test_gpu_quant_stack.py).
 *
 * Semantics: layer l with quant = q is sgx_layer_forward with desc->quant = q and gat_fill_dead_rows = 0 on the same
 * operands in fp32 (quant = NULL: the plain layer of sgx_gat_stack_forward).  Operands arrive UNQUANTISED and each is
 * quantised exactly once (the quantiser is not idempotent: inv_scale_w = 127 against a grid step of 1 / 128 at 8 bits),
 * with the one device quantiser of sgx_fake_quantize, so the bits are those of a sgx_fake_quantize launch over them:
 *   - B and attention go to the signed q->qbits grid (inv_scale_w, zero_w) as the kernel loads them;
 *   - X_l goes to the unsigned grid with (inv_scale_fea, zero_fea) of layer l: the stored CSR entries of a sparse layer 0
 *     as they are read, a dense layer 0 as it is copied into LDS, and for l >= 1 the previous layer's D_{l-1} where the
 *     aggregate stores it into the X tile -- the value written to the caller's layer[l-1].D is the unquantised D_{l-1},
 *     and the last layer's tile stays unquantised for the readout;
 *   - adjacency values go to the unsigned grid with (inv_scale_adj, zero_adj) as they are read, or are taken as stored
 *     with SGX_QUANT_ADJ_DONE; in a GAT layer the mask is on the quantised value (> 0 is live);
 *   - H_l = requant(X_q . W_q): the shift by scale_fea, the clip to +-(2^ib - 1) / 2^ib and the decimal rounding that
 *     sgx_xw_dense / sgx_xw_sparse apply on their stores (one fp32 operation per rounding point, contraction off);
 *   - D_l = act(aggregate) * deq_factor: ReLU first, then the scale; GAT rows without a live entry give 0;
 *   - readout and head: those of sgx_stack_forward.
 * The stack always takes the fp32 form: SGX_QUANT_INT8 and SGX_QUANT_INT8_AUTO in `flags` are ignored.  Fields of
 * sgx_quant read on the fused path: qbits, scale_fea, internal_bits, flags (SGX_QUANT_ADJ_DONE only), the three
 * (inv_scale, zero) pairs and deq_factor; nnz_adj and nnz_fea are not needed there.  The chained path hands the block
 * to sgx_layer_forward, which sizes its quantised copies by them: nnz_adj (unless SGX_QUANT_ADJ_DONE) and, for a sparse
 * layer 0, nnz_fea must then hold the stored entries of A and X.
 *
 * GCN layers are bit-equal to the chain sgx_layer_forward x n -> sgx_readout_mean_linear wherever X_q . W_q is exact in
 * fp32 (|sum of code products| < 2^24: every M_fea <= 256 at 8 bits), the aggregate being the same fma chain in CSR
 * order; GAT layers lie inside the bound of sgx_gat_stack_forward times deq_factor.  Same bits on every run and for every
 * grouping: no atomics, no order that depends on the grid.  LDS use and the row budget are those of
 * sgx_gat_stack_forward in fp32.
 *
 * Where the plan does not fit or a width is over the limit the call runs, per layer, sgx_layer_forward with the layer's
 * quant (gat_fill_dead_rows = 0, no plan), then sgx_readout_mean_linear, all through the workspace, so a call always
 * works; sgx_quant_stack_workspace_bytes is 0 exactly when the fused path is taken.  A descriptor with every quant NULL
 * is exactly sgx_gat_stack_forward.
 *
 * Argument errors, returned before anything reaches the device: those of sgx_gat_stack_forward; a layer with quant set
 * while dtype != SGX_F32, qbits outside {8, 4, 2, 1}, scale_fea outside 0..30, internal_bits outside 1..30, zero_adj
 * != 0, or zero_fea != 0 on a sparse layer 0 (entries that are not stored must stay zero): SGX_ERR_UNSUPPORTED.
 * Capturable on the fused path: no allocation and no host synchronisation. */
typedef struct sgx_quant_stack_layer {
    int32_t gemm_mode;    /* as sgx_gat_stack_layer, field for field */
    int32_t relu;
    int32_t M_fea, P_w;
    const void *B;
    void *D;
    int64_t ldd;
    int32_t gat_mode;
    const void *attention;
    float alpha;
    const sgx_quant *quant;   /* this layer's quantiser; NULL = the plain layer of sgx_gat_stack_forward */
} sgx_quant_stack_layer;

typedef struct sgx_quant_stack_desc {
    int32_t dtype, n_layers;                   /* as sgx_gat_stack_desc, field for field */
    int32_t n_rows, n_graphs;
    const int32_t *graph_ptr;
    const int32_t *rowPtr_adj, *columnIndex_adj; const void *values_adj;
    const int32_t *rowPtr_fea, *columnIndex_fea; const void *values_fea;
    sgx_quant_stack_layer layer[4];
    int32_t C;
    const float *W_head, *bias;
    float *pooled, *logits;
    const sgx_batch_plan *plan;                /* from sgx_batch_plan_create / _create_ex / _create_known, either kind */
    void *workspace; size_t workspace_bytes;   /* sgx_quant_stack_workspace_bytes(d), 256-byte aligned (0 on the fused path) */
} sgx_quant_stack_desc;

/* 0 for the fused path, the chained path's scratch otherwise (and for a bad descriptor) */
size_t sgx_quant_stack_workspace_bytes(const sgx_quant_stack_desc *d);
int sgx_quant_stack_forward(const sgx_quant_stack_desc *d, void *stream);

/* ---- training the GAT stack ---------------------------------------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_gat_stack_backward is sgx_stack_backward with a per-layer choice of the matrix P in G_l = P . g_l: the adjacency
 * (gat_mode 0) or the layer's attention matrix S (gat_mode 1), as the reference's FPYNQ_GAT.backward multiplies --
 * grad_input = P (g W^T), grad_weights = X^T (P g), P and never P^T -- plus the gradient of the attention vector.  Every
 * sum stays inside one graph, so inside one workgroup.  Parity of the GAT layer is UNPINNED: the reference records no GAT
 * output; what is pinned is the float64 restatement of tests/_gat_stack_grad_ref.py.
 *
 * Plans: an SGX_BATCH_BACKWARD plan exactly as sgx_stack_backward takes it (same row budget R, same groups): one plan
 * cached on a batch serves sgx_gat_stack_forward, sgx_stack_backward and this call.  Beside sgx_stack_backward's three
 * tiles a row the kernel keeps Wh in fp32 and six floats (s1, s2, m, 1 / l, rs, g1): the launch asks for
 * R x (grad_row_bytes + 4 lds_pitch(fp32, max_width) + 24) bytes of dynamic LDS (sgx_gat_stack_backward_lds_bytes; fp16
 * at width 64: R = 80, 78 720 B; fp32 at width 256: R = 16, 66 944 B; under 100 KiB at every dtype and width), and
 * SGX_ERR_UNSUPPORTED should that ever pass the 160 KiB a workgroup may declare.
 *
 * Semantics, per group of graphs, layers from the top down; g_{L-1}, the ReLU mask (where relu is set and D_l == 0) and
 * the rounding of a handed-down gradient to dtype are sgx_stack_backward's:
 *   gat_mode = 0: sgx_stack_backward's layer; G_l is bit-equal to it.
 *   gat_mode = 1: the forward quantities are formed again from X_l (layer 0's features, or D_{l-1} as stored in dtype)
 *     and the fp32 parameters:
 *       Wh  = fp32(X_l) . W_l          fp32: dense layers in the MFMA layout and K order of sgx_xw_dense's fp32 kernel, a
 *                                      sparse layer 0 by the fma chain in CSR order
 *       s1  = Wh . a1, s2 = Wh . a2;   E_e = LeakyReLU_alpha(s1_i + s2_c) on every stored entry e = (i, c)
 *       an entry is live iff values[e] > 0; m_i and l_i over the row's live entries;
 *       S_e = exp(E_e - m_i) / l_i on live entries, 0 on masked ones
 *     then, as sgx_gat_backward_edges:
 *       d_e = g_i . Wh_c;  dx_e = S_e d_e;  rs_i = sum_row dx
 *       sg_e = (dx_e - S_e rs_i) (E_e > 0 ? 1 : alpha), 0 on masked entries;  g1_i = sum_row sg
 *       G_l = sum_e S_e g_c  (P . g);   T_i = sum_e sg_e Wh_c
 *       grad_attention = [sum_i g1_i Wh_i ; sum_i T_i]     (sgx_gat_attention_grad's row-order form)
 *       dW_l = X_l^T G_l;   g_{l-1} = dtype(G_l W_l^T), then the mask of layer l - 1
 *     A row without a live entry has S = 0 on every entry and contributes nothing (the stack's zero rule; the
 *     mean-of-all-rows rule is not offered).  One head.
 * dW_l and grad_attention are summed as sgx_stack_backward sums dW: every workgroup of a persistent grid of
 * min(max(groups, 1), 512) adds its groups (rows in order) into its own fp32 slice of the workspace with plain loads and
 * stores, and a second launch adds the slices in slice order -- no atomics, the same bits on every run.  The summation
 * order of the attention path is fixed by the layer's width alone and is not pinned to the chained kernels'.
 *
 * Limits: those of sgx_stack_backward.  No chained form inside the call: the model's layer-by-layer path is that form.
 * Capturable: no allocation and no host synchronisation.
 *
 * Argument errors, returned before anything reaches the device: those of sgx_stack_backward; attention or
 * grad_attention NULL on a layer with gat_mode = 1: SGX_ERR_NULL; gat_mode outside {0, 1}, a forward-kind plan:
 * SGX_ERR_UNSUPPORTED.  n_rows == 0: every gradient is set to zero. */
typedef struct sgx_gat_stack_grad_layer {
    int32_t gemm_mode;    /* as sgx_stack_grad_layer, field for field */
    int32_t relu;
    int32_t M_fea, P_w;
    const float *W;
    const void *D;
    int64_t ldd;
    float *grad_W;
    float *G;
    int32_t gat_mode;         /* 0: P = the adjacency; 1: P = the edge softmax above */
    const float *attention;   /* gat_mode = 1: the fp32 parameter [2 * P_w], a1 then a2 */
    float alpha;              /* LeakyReLU slope of the scores */
    float *grad_attention;    /* gat_mode = 1, out: [2 * P_w] fp32 */
    float *S, *E;             /* gat_mode = 1, optional outs: [nnz_adj] fp32 (NULL = not written) */
} sgx_gat_stack_grad_layer;

typedef struct sgx_gat_stack_grad_desc {
    int32_t dtype, n_layers;                   /* as sgx_stack_grad_desc, field for field */
    int32_t n_rows, n_graphs;
    const int32_t *graph_ptr;
    const int32_t *rowPtr_adj, *columnIndex_adj; const void *values_adj;
    const int32_t *rowPtr_fea, *columnIndex_fea; const void *values_fea;
    sgx_gat_stack_grad_layer layer[4];
    const float *grad_pooled;
    const sgx_batch_plan *plan;                /* an SGX_BATCH_BACKWARD plan */
    void *workspace; size_t workspace_bytes;   /* sgx_gat_stack_backward_workspace_bytes(d), 256-byte aligned */
} sgx_gat_stack_grad_desc;

/* the gradient slices: min(max(groups, 1), 512) x (sum_l M_fea P_w + sum over GAT layers 2 P_w) floats, every block
 * padded to 16 bytes; 0 for a descriptor the call refuses */
size_t sgx_gat_stack_backward_workspace_bytes(const sgx_gat_stack_grad_desc *d);
/* informational: the dynamic LDS of the launch in bytes, computed on the host (no caller needs it to make the call; the
 * tests check the formula above with it); 0 for a descriptor the call refuses */
size_t sgx_gat_stack_backward_lds_bytes(const sgx_gat_stack_grad_desc *d);
int sgx_gat_stack_backward(const sgx_gat_stack_grad_desc *d, void *stream);

/* ---- training the quantised stack ---------------------------------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_quant_stack_backward is sgx_gat_stack_backward with a per-layer quantiser: the backward of the stack that
 * sgx_quant_stack_forward runs, by the rule of the reference's FPYNQ_GAT.backward under fake quantisation -- "the
 * backward pass uses the unquantised operands".  The attention matrix of a quantised GAT layer is the QUANTISED
 * forward's S, formed again in the kernel; everything a gradient multiplies with is unquantised.  Parity of the
 * quantised layer is UNPINNED; what is pinned is the float64 restatement of tests/_quant_stack_grad_ref.py.
 *
 * Plans, LDS, workspace: the same SGX_BATCH_BACKWARD plan as sgx_stack_backward and sgx_gat_stack_backward, the LDS
 * formula of sgx_gat_stack_backward_lds_bytes (H_q and the unquantised Wh share one tile), the same gradient slices and
 * reduction launch.  No atomics, no order that depends on the grid, capturable.  No chained form inside the call.
 *
 * Semantics, per layer l from the top down; g_{L-1}, the ReLU mask (relu set and D_l == 0) and the rounding of
 * handed-down gradients are sgx_stack_backward's.  D_l is the quantised forward's output, act(aggregate) * deq_factor, as
 * sgx_quant_stack_forward stored it; deq_factor is applied to no gradient (straight-through):
 *   gat_mode = 0, quantised or not: P is the UNQUANTISED adjacency (values_adj), X_l the unquantised input (layer 0's
 *     features, or D_{l-1} as stored), W_l the fp32 parameter: sgx_stack_backward's layer, G_l bit-equal to it.
 *   gat_mode = 1 with quant = q:
 *     1. H_q = requant(X_q . W_q) as sgx_quant_stack_forward forms it: X on the unsigned grid with layer l's
 *        (inv_scale_fea, zero_fea), W on the signed grid, then the shift by scale_fea, the clip and the decimal
 *        rounding; one device quantiser statement per rounding point, contraction off; pad elements stay 0.
 *     2. s1 = H_q . a1_q, s2 = H_q . a2_q with the attention vector on the signed grid; E_e = LeakyReLU(s1_i + s2_c);
 *        an entry is live iff its QUANTISED adjacency value is > 0 -- values_adj_q[e] as stored where q->flags has
 *        SGX_QUANT_ADJ_DONE, values_adj[e] quantised with (inv_scale_adj, zero_adj) as it is read otherwise; m_i, l_i
 *        and S_e as in sgx_gat_stack_backward.
 *     3. Wh = fp32(X_l) . W_l UNQUANTISED, written over H_q's LDS tile (H_q is dead once s1, s2, m and 1 / l exist).
 *     4. sgx_gat_stack_backward's passes on S, E and the unquantised Wh: G_l = sum_e S_e g_c; sg, g1 and T;
 *        grad_attention = [sum_i g1_i Wh_i ; sum_i T_i]; dW_l = X_l^T G_l; g_{l-1} = dtype(G_l W_l^T).
 *     A row without a live entry contributes nothing (the stack's zero rule).
 *   quant = NULL: sgx_gat_stack_backward's layer bit for bit; a descriptor without a quantised GAT layer is that call.
 * Fields of sgx_quant read: qbits, scale_fea, internal_bits, flags (SGX_QUANT_ADJ_DONE only), the three (inv_scale,
 * zero) pairs.
 *
 * Argument errors, returned before anything reaches the device: those of sgx_gat_stack_backward; a layer with quant set
 * while dtype != SGX_F32, qbits outside {8, 4, 2, 1}, scale_fea outside 0..30, internal_bits outside 1..30, zero_adj
 * != 0, or zero_fea != 0 on a sparse layer 0: SGX_ERR_UNSUPPORTED; a GAT layer with SGX_QUANT_ADJ_DONE while
 * values_adj_q == NULL: SGX_ERR_NULL.  n_rows == 0: every gradient is set to zero. */
typedef struct sgx_quant_stack_grad_layer {
    int32_t gemm_mode;    /* as sgx_gat_stack_grad_layer, field for field */
    int32_t relu;
    int32_t M_fea, P_w;
    const float *W;
    const void *D;
    int64_t ldd;
    float *grad_W;
    float *G;
    int32_t gat_mode;
    const float *attention;
    float alpha;
    float *grad_attention;
    float *S, *E;
    const sgx_quant *quant;   /* this layer's quantiser; NULL = the plain layer of sgx_gat_stack_backward */
} sgx_quant_stack_grad_layer;

typedef struct sgx_quant_stack_grad_desc {
    int32_t dtype, n_layers;                   /* as sgx_gat_stack_grad_desc, field for field */
    int32_t n_rows, n_graphs;
    const int32_t *graph_ptr;
    const int32_t *rowPtr_adj, *columnIndex_adj; const void *values_adj;   /* the UNQUANTISED adjacency */
    const int32_t *rowPtr_fea, *columnIndex_fea; const void *values_fea;
    sgx_quant_stack_grad_layer layer[4];
    const float *grad_pooled;
    const sgx_batch_plan *plan;                /* an SGX_BATCH_BACKWARD plan */
    void *workspace; size_t workspace_bytes;   /* sgx_quant_stack_backward_workspace_bytes(d), 256-byte aligned */
    const float *values_adj_q;                 /* [nnz_adj] fp32, the quantised adjacency: what a GAT layer whose quant has
                                                  SGX_QUANT_ADJ_DONE masks with; NULL where no layer has the flag */
} sgx_quant_stack_grad_desc;

/* sgx_gat_stack_backward_workspace_bytes' and _lds_bytes' formulas; 0 for a descriptor the call refuses */
size_t sgx_quant_stack_backward_workspace_bytes(const sgx_quant_stack_grad_desc *d);
size_t sgx_quant_stack_backward_lds_bytes(const sgx_quant_stack_grad_desc *d);
int sgx_quant_stack_backward(const sgx_quant_stack_grad_desc *d, void *stream);

/* ---- the loss head: dropout, the Linear head, cross entropy and their gradients in one call --------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_head_loss is the classifier tail of GCN_PYNQ / GAT_POOL_PYNQ behind the pooled means -- dropout(p), Linear
 * [C][P], CrossEntropyLoss(reduction = mean) -- with its whole gradient: grad_pooled for the stack's backward, grad_W
 * and grad_bias for the optimiser.  All arrays fp32 on the device, target int64.  u64 arithmetic wraps.
 *   step_total = step + (step_dev ? (uint64)step_dev[0] : 0)            step_dev is read on the device, by the launch
 *   dropout    k = mix64(mix64(mix64(seed) ^ step_total) ^ (uint64)(g * P + j))       mix64: the sampler's, above
 *              keep(g, j) iff (k >> 40) >= floor(p * 2^24)              the hash's top 24 bits against p as a float's value
 *              scale = 1.0f / (1.0f - p)                                two fp32 operations, formed once
 *              x[g][j] = keep ? pooled[g][j] * scale : 0                p == 0: every element kept, x == pooled bit for bit
 *   logits     z[g][c] = bias[c] + sum_j W[c][j] x[g][j] in sgx_readout_mean_linear's order: 64 lanes, lane l an fmaf
 *              chain from 0 over j = l, l + 64, ...; the lanes added by the xor butterfly 32, 16, .. 1; then + bias[c]
 *              (0 without a bias).  At p == 0 bit-equal to sgx_readout_mean_linear on one-row graphs.
 *   loss       m = max_c z_c;  lse = m + logf(sum_c expf(z_c - m)), c ascending from 0;  loss_g = lse - z[target_g]
 *              loss = (sum over slices b ascending of (sum of loss_g over g = b, b + S, ... ascending)) / (float)G
 *   gradients  gs = grad_scale / (float)G
 *              dz[g][c] = (expf(z_c - lse) - (c == target_g ? 1 : 0)) * gs
 *              grad_pooled[g][j] = keep ? scale * (fmaf chain from 0 over c ascending of dz[g][c] * W[c][j]) : 0
 *              grad_W[c][j] = sum_g dz[g][c] x[g][j];  grad_bias[c] = sum_g dz[g][c]
 * A target outside [0, C) gives loss_g = 0 and dz[g][.] = 0 and indexes nothing; the divisor stays G.
 * Sums over graphs are the only sums across workgroups, done as sgx_stack_backward does its weight gradients: S =
 * min(G, 256) workgroups whatever the device; workgroup b adds its graphs b, b + S, ... in that order into its own fp32
 * slice of the workspace (an fmaf on the slice's previous value for grad_W, an add for grad_bias and the loss; the first
 * graph stores; plain loads and stores, no atomics), and a second launch adds the slices from 0 in slice order.  The same
 * bits on every run and every device.
 *
 * Limits: P <= 1024, C <= 64; beyond: SGX_ERR_UNSUPPORTED.  Capturable: no allocation, no synchronisation.
 * Argument errors, returned before anything reaches the device: n_graphs, P or C below 1: SGX_ERR_SHAPE; pooled, W,
 * target, loss, grad_pooled or grad_W NULL, grad_bias NULL with a bias: SGX_ERR_NULL (bias NULL: grad_bias is not
 * written; logits NULL: not written); p outside [0, 1) or over a limit: SGX_ERR_UNSUPPORTED; workspace missing or
 * below sgx_head_loss_workspace_bytes: SGX_ERR_WORKSPACE; not 256-byte aligned: SGX_ERR_ALIGN. */
/* min(G, 256) * (C * P + C + 1) floats, rounded up to 256 bytes; 0 for a shape the call refuses */
size_t sgx_head_loss_workspace_bytes(int n_graphs, int P, int C);
int sgx_head_loss(int n_graphs, int P, int C, const float *pooled, const float *W, const float *bias,
                  const int64_t *target, float p_drop, uint64_t seed, uint64_t step, const int64_t *step_dev,
                  float grad_scale, float *loss, float *logits, float *grad_pooled, float *grad_W, float *grad_bias,
                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- the optimiser: multi-tensor Adam on a device step counter ---------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_adam_step is torch.optim.Adam (no amsgrad, weight_decay as L2 added to the gradient) on up to
 * SGX_ADAM_MAX_TENSORS fp32 tensors in one launch; the tensor table travels in the kernel arguments.  The step counter
 * is a device int64: the call reads t - 1 from it, uses t, and a trailing one-thread launch leaves t there -- one
 * captured call is the right update at every replay.  Per element, every operation an individually rounded fp32 one
 * (no contraction), the constants rounded once from the doubles of the descriptor:
 *     b1 = (float)beta1, ob1 = (float)(1 - beta1), b2 = (float)beta2, ob2 = (float)(1 - beta2)     (1 - beta in double)
 *     bc1 = (float)(1 - pow(beta1, t)),  sqrt_bc2 = (float)sqrt(1 - pow(beta2, t))                  (in double, then rounded)
 *     step_size = (float)lr / bc1
 *     g = grad;  weight_decay != 0:  r = (float)weight_decay * param;  g = g + r
 *     m = b1 * m + ob1 * g                  (two products, one sum)
 *     v = b2 * v + ob2 * (g * g)            (three products, one sum)
 *     denom = sqrtf(v) / sqrt_bc2 + (float)eps
 *     param = param - step_size * (m / denom)
 * param, m, v are updated in place.  A tensor with n == 0 or grad == NULL is skipped, as torch skips p.grad is None.
 * param_t_out (optional): the updated parameter seen as [rows][cols] row-major, written transposed [cols][rows] and
 * cast to dtype_t -- bit-equal to torch.transpose(param, 0, 1).to(dtype).contiguous() on the updated parameter, the
 * W^T a stack forward takes.
 *
 * Capturable: no allocation, no synchronisation.  Argument errors, returned before anything reaches the device: d or
 * step NULL, param / m / v NULL on a tensor that is not skipped: SGX_ERR_NULL; n_tensors outside 0 ..
 * SGX_ADAM_MAX_TENSORS, n < 0, param_t_out with rows * cols != n: SGX_ERR_SHAPE; a negative or NaN hyper-parameter,
 * a beta outside [0, 1), a dtype_t other than SGX_F16 / SGX_F32: SGX_ERR_UNSUPPORTED. */
#define SGX_ADAM_MAX_TENSORS 16

typedef struct sgx_adam_tensor {
    float *param, *m, *v;        /* [n] fp32, updated in place */
    const float *grad;           /* [n] fp32; NULL = the tensor is skipped */
    int64_t n;                   /* elements; 0 = skipped */
    void *param_t_out;           /* optional [cols][rows] in dtype_t */
    int32_t dtype_t, rows, cols; /* read only with param_t_out */
} sgx_adam_tensor;

typedef struct sgx_adam_desc {
    int32_t n_tensors;           /* 0 .. SGX_ADAM_MAX_TENSORS */
    double lr, beta1, beta2, eps, weight_decay;
    int64_t *step;               /* device: t - 1 on entry, t after the call's launches */
    sgx_adam_tensor tensor[SGX_ADAM_MAX_TENSORS];
} sgx_adam_desc;

int sgx_adam_step(const sgx_adam_desc *d, void *stream);

/* ---- the node loss head: the loss head over selected rows of a node matrix ----------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_node_loss is the classifier tail of GAT_PYNQ's training loop behind the last layer -- dropout(p), Linear [C][P],
 * CrossEntropyLoss(reduction = mean) over out[train] / out[batch.train_mask] / out[:batch_size] -- with its whole
 * gradient, the selected rows' count and the arg-max's hits.  All arrays fp32 on the device, H [n_rows][P], W [C][P],
 * target int64 [n_rows], mask bytes [n_rows] (a bool array as its bytes).  u64 arithmetic wraps.
 *   selection  row i is selected iff i < n_prefix && (mask == NULL || mask[i] != 0).  M = the number of selected rows,
 *              counted on the device by a launch of its own (integer partial counts); the host never learns it.
 *              n_prefix = n_rows with a mask: the full graph; n_prefix = batch_size without one: a seeds-first batch.
 *   dropout    sgx_head_loss's exactly, element (i, j) at index i * P + j, step_total = step + step_dev[0]:
 *              keep(i, j), scale = 1.0f / (1.0f - p), x[i][j] = keep ? H[i][j] * scale : 0; p == 0: x == H bit for bit
 *   logits     z[i][c] = (fmaf chain from 0 over j ascending from 0 of W[c][j] * x[i][j]) + bias[c]     (0 without a bias)
 *   per selected row:  m = max_c z_c;  lse = m + logf(sum_c expf(z_c - m)), c ascending from 0;  loss_i = lse - z[target_i]
 *              gs = grad_scale / (float)M
 *              dz[i][c] = (expf(z_c - lse) - (c == target_i ? 1 : 0)) * gs
 *              a target outside [0, C): loss_i = 0, dz[i][.] = 0, nothing is indexed, the row is not a hit; it counts in M
 *              hit_i: arg-max of z[i] == target_i, the arg-max over c ascending with a strict > from z[0] (a NaN z[0]
 *              counts as -inf): the lowest index wins a tie, a NaN never wins
 *   unselected rows have dz = 0 and take part in no sum
 *   grad_H[i][j] = keep ? scale * (fmaf chain from 0 over c ascending of dz[i][c] * W[c][j]) : 0   for EVERY i < n_rows;
 *              exact zeros in unselected rows
 *   sums over rows: rows are cut into blocks of SGX_NODE_LOSS_ROWS consecutive rows; block b belongs to slice b mod S,
 *              S = min(number of blocks, SGX_NODE_LOSS_GRID) whatever the device.  Within a slice, blocks ascending:
 *              grad_W[c][j]: ONE fmaf chain from 0 over the slice's selected rows in ascending row order of dz[i][c] * x[i][j]
 *              grad_bias[c]: one chain of additions from 0 over the same rows in the same order
 *              loss: per row position r = i mod SGX_NODE_LOSS_ROWS a chain of additions from 0 over the slice's
 *              selected rows at that position, ascending; then the positions r = 0, 1, .. added from 0
 *              Then the slices are added from 0 in slice order (fp32 additions), and loss = sum / (float)M.
 *              Plain loads and stores, no floating-point atomics: the same bits on every run and every device.
 *   M == 0     loss = 0 and every gradient 0 (torch gives NaN for the mean over no row).
 *   counts     optional, int64 [2] = {M, hits}.   logits: optional, z for every i < n_rows, selected or not.
 *   grad_H, grad_W and grad_bias all NULL: evaluation mode -- loss, counts and logits only; a row that feeds none of
 *              them is not read.  In either mode a block without a needed row (selected, or any row when logits are
 *              wanted) is not read either: its grad_H rows are zero-filled.
 * Limits: P <= 1024, C <= 64, C * P <= 16384 (64 accumulators a thread, 64 KiB of W in LDS); beyond: SGX_ERR_UNSUPPORTED
 * and a workspace size of 0.  Capturable: no allocation, no synchronisation (three kernel nodes).
 * Argument errors, returned before anything reaches the device: n_rows, P or C below 1, n_prefix < 0: SGX_ERR_SHAPE; H, W,
 * target or loss NULL, or only part of grad_H / grad_W / grad_bias NULL (grad_bias is required exactly when bias is
 * given; without a bias it is not written): SGX_ERR_NULL; p outside [0, 1) or over a limit: SGX_ERR_UNSUPPORTED;
 * workspace missing or below sgx_node_loss_workspace_bytes: SGX_ERR_WORKSPACE; not 256-byte aligned: SGX_ERR_ALIGN. */
#define SGX_NODE_LOSS_ROWS 16
#define SGX_NODE_LOSS_GRID 512

/* 2048 + min(ceil(n_rows / SGX_NODE_LOSS_ROWS), SGX_NODE_LOSS_GRID) * (C * P + C + 2) floats rounded up to 256 bytes; 0 for
 * a shape the call refuses */
size_t sgx_node_loss_workspace_bytes(int64_t n_rows, int P, int C);
int sgx_node_loss(int64_t n_rows, int64_t n_prefix, int P, int C, const float *H, const float *W, const float *bias,
                  const int64_t *target, const uint8_t *mask, float p_drop, uint64_t seed, uint64_t step,
                  const int64_t *step_dev, float grad_scale, float *loss, int64_t *counts, float *logits, float *grad_H,
                  float *grad_W, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the evaluation head: hits and the summed loss of a pass, kept on the device across batches --------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_head_eval is the evaluation of GCN_PYNQ / GAT_POOL_PYNQ behind the pooled means -- Linear [C][P], arg-max against
 * the label, CrossEntropyLoss(reduction = sum) -- for one batch of a pass over a loader.  It ADDS to accumulators the
 * caller zeroes once per pass, so batches of unequal size accumulate on the device and a pass is read back once
 * (sgx_node_loss's counts are overwritten per call and its loss is that call's mean).  pooled [n_graphs][P], W [C][P],
 * bias [C] or NULL fp32, target int64 [n_graphs], all on the device.  Rows n_real .. n_graphs - 1 are the filler graphs
 * of a padded batch.
 *   logits     z[g][c] of sgx_head_loss with p_drop = 0, bit for bit (x == pooled; 64 lanes, lane l an fmaf chain from
 *              0 over j = l, l + 64, ...; the xor butterfly 32, 16, .. 1; then + bias[c], 0 without a bias)
 *   per row g < n_real:  sgx_head_loss's per-row term, bit for bit: m = max_c z_c;  lse = m + logf(sum_c expf(z_c - m)),
 *              c ascending from 0;  loss_g = lse - z[target_g]
 *              hit_g: arg-max of z[g] == target_g, sgx_node_loss's arg-max: over c ascending with a strict > from z[0]
 *              (a NaN z[0] counts as -inf): the lowest index wins a tie (torch's rule), a NaN never wins
 *              a target outside [0, C): loss_g = 0, no hit, nothing is indexed; the row still counts in totals[0]
 *   the call adds:  totals[0] += n_real;  totals[1] += sum_g hit_g;
 *              loss_sum[0] += (double)loss_0 + (double)loss_1 + ... : the rows' fp32 losses added from 0.0 in row order
 *              in double, and that double added to loss_sum[0] once
 *   rows n_real .. n_graphs - 1 are never read for the sums (they may hold anything, NaN included); without `logits` they
 *              are not read at all.  logits, when given, receives all n_graphs rows.
 *   n_real = 0 is valid: nothing is added; only `logits` is written.
 * Two launches, as sgx_head_loss: a wavefront per row, every row's loss to a slot of its own in the workspace and the
 * hit counts (integers) per wavefront, so nothing that is summed depends on the grid; then one workgroup adds the slots
 * in row order and adds to the accumulators.  No atomics: the same bits on every run, for any grid and on every device.
 * Capturable: no allocation, no synchronisation.  The accumulators are read and written by the launch, on the stream.
 *
 * Limits: sgx_head_loss's, P <= 1024, C <= 64; beyond: SGX_ERR_UNSUPPORTED and a workspace size of 0.
 * Argument errors, returned before anything reaches the device: n_graphs, P or C below 1, n_real outside 0 .. n_graphs:
 * SGX_ERR_SHAPE; pooled, W, target, totals or loss_sum NULL: SGX_ERR_NULL (bias NULL: no bias; logits NULL: not
 * written); over a limit: SGX_ERR_UNSUPPORTED; workspace missing or below sgx_head_eval_workspace_bytes:
 * SGX_ERR_WORKSPACE; not 256-byte aligned: SGX_ERR_ALIGN. */
/* 256 + n_graphs floats rounded up to 256 bytes + 4096; 0 for a shape the call refuses */
size_t sgx_head_eval_workspace_bytes(int n_graphs, int P, int C);
int sgx_head_eval(int n_graphs, int n_real, int P, int C, const float *pooled, const float *W, const float *bias,
                  const int64_t *target, int64_t *totals /* [2] */, double *loss_sum /* [1] */, float *logits /* or NULL */,
                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- padded node batches: every full batch of a loader in buffers of one fixed capacity -------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * A neighbour-sampled batch has its own node, edge and entry counts; sgx_node_batch_sample reads them back, and they are
 * tensor sizes and launch arguments of everything behind it, so a recorded step fits one batch.  A PADDED node batch has
 * the counts of a capacity the host computes once per (graph, batch, fanouts, feature CSR), the spare rows and entries
 * held by well-defined filler rows; one recorded step then serves every batch of `batch` seeds.
 *
 * Capacity (sgx_node_batch_pad_capacity; host arithmetic only).  mn, me = the bounds max_nodes, max_edges of
 * sgx_node_batch_workspace_bytes:
 *   C_f   the feature entries: the sum of the mn largest per-row entry counts of the whole graph's feature CSR
 *         (fea_row_counts, HOST [n_nodes]; NULL: no features, C_f = 0);
 *   F     max(ceil(me / 63), ceil(C_f / 64)) guaranteed filler rows;
 *   N     mn + F rows of every padded array;       E = me entries of a row of the edge lists;
 *   C_a   me + mn + F = me + N entries of the normalised adjacency.
 * Every batch fits.  A batch with n live rows, `edges` sampled edges, a adjacency and f feature entries has n <= mn and
 * edges <= me (the sampler's bounds), n <= a <= edges + n (a row gets one loop unless it stores one) and f <= C_f (its n
 * distinct nodes hold no more than the mn fullest rows).  It leaves P = N - n >= F filler rows, which take one diagonal
 * entry each; the spare adjacency entries are C_a - a - P = me + n - a, within 0 .. me <= 63 F <= 63 P, and the spare
 * feature entries C_f - f are within 0 .. C_f <= 64 F <= 64 P: dealt 63 / 64 to a row they end inside the filler rows.
 *
 * A padded batch holds, in the live prefix of every array, exactly what sgx_node_batch_sample writes for the same (graph,
 * seeds, fanouts, seed, step), bit for bit -- n_id, out_rowPtr / out_col / edge_pos, rowPtr_norm / columnIndex_norm /
 * values_norm, dead_row, rowPtr_fea / columnIndex_fea / values_fea, y_out, mask_out, and the two edge lists as int64
 * [2][E]: row 1 begins at entry E, not at `edges` -- and behind the prefix:
 *   filler row n+j  n_id = -1, y_out = 0, every mask byte 0, dead_row = 0; whoever gathers dense x rows by n_id gives it a
 *                   row of zeros (sgx_pack_rows: a negative index is a zero row);
 *     adjacency     one diagonal entry (n + j, 1), then zero-valued diagonal entries (n + j, 0): the S_a = C_a - a - P
 *                   spare entries dealt 63 to a row from filler row 0 on, so the row holds 1 + clamp(S_a - 63 j, 0, 63)
 *                   entries: rowPtr_norm[n + j] = a + j + min(S_a, 63 j), rowPtr_norm[N] = C_a;
 *     features      zero-valued entries (0, 0): the S_f = C_f - f spare entries dealt 64 to a row from filler row 0 on:
 *                   rowPtr_fea[n + j] = f + min(S_f, 64 j), rowPtr_fea[N] = C_f;
 *     sampled CSR   empty: out_rowPtr[n .. N] = edges;
 *   tails           out_col, edge_pos [edges, E) = -1; edge_index[:, edges:E] = -1 and edge_index_agg likewise (past the
 *                   live edges a padded edge list is a key, not an edge list).
 * Every stored entry of the normalised adjacency and of the feature CSR belongs to a row -- rowPtr[N] is the array's
 * length in every batch -- so code that takes a CSR's entry count from its column array runs on them unchanged.
 * Consequences: the longest row of the normalised adjacency is at most max(max(fanouts) + 1, 64) and of the feature CSR
 * max(its longest row, 64); no filler row is dead under the GAT mask `adj > 0` (its first entry is 1); a filler row's D
 * is 0 in every layer (X.W of a zero row is 0, and the row aggregates itself alone); no live row stores a filler
 * column, so a filler row passes nothing on, and a loss over live rows hands it no gradient.  One exception is inherited
 * from the layers: a DEAD live row of the GAT aggregate takes the uniform softmax over all N columns, fillers included
 * (they add 0 to the sum; the mean divides by N, not n).
 *
 * sgx_node_batch_sample_padded(b, pad, stream): the launches of sgx_node_batch_sample on b's arguments with
 *   pad->step    (device, uint64) in place of b->step: the sampling key is formed in the kernels from this word -- the
 *                same key as the host forms for the same value -- so a replay draws a new sample once the word changes;
 *   pad->status  (device, int32) |= the sampler's status word (1: bad or repeated seeds, 2: a capacity); never read back
 *                by the call;
 *   pad->counts  (device, int32 [4 + 2 (n_hops + 1)]) = n, edges, a, f, then the node count and the edge count after
 *                every hop (hop_nodes, hop_edges), for tests and reports;
 * and one more launch whose workgroups write the filler rows, the dealt spare entries and the tails: plain stores,
 * 16 bytes a lane over the constant ranges, no atomics beyond the sampler's.  Array sizes: n_id, dead_row, y_out,
 * mask_out [N]; the three row pointers [N + 1]; out_col, edge_pos [E]; columnIndex_norm, values_norm [C_a];
 * columnIndex_fea, values_fea [C_f] (b->fea_capacity is ignored); the edge lists [2 E]; b->max_nodes / max_edges and the
 * workspace as for sgx_node_batch_sample.  Nothing in *b is written: hop_nodes, hop_edges (may be NULL), nnz_norm,
 * nnz_fea, has_dead_rows and max_row stay as they are.  No allocation, no synchronisation; capturable; the same bits on
 * every run.  With a non-zero status the arrays hold a batch without a live row (n = edges = a = f = 0 in counts:
 * filler rows only), so whatever runs behind the call reads a well-formed batch; nothing is written outside
 * [0, capacity) of any array.
 *
 * sgx_node_batch_sample_padded_quant(b, pad, q, stream): the padded batch ready for the QUANTISED layers.  It is
 * sgx_node_batch_sample_padded(b, pad) -- the same launches, the same bits in every array that call writes, the same
 * status, counts and step word -- and for each constant set k < q->n_sets (sgx_node_batch_quant above) it also writes, with
 * fq_k the unsigned-grid device function sgx_fake_quantize(0, qbits, inv_scale_adj[k], zero_adj[k]) runs
 * (csrc/quant_device.h, the one quantiser):
 *   values_q[k][e]    = fq_k(values_norm[e]) for every e < C_a, the whole capacity: the live prefix holds the bits
 *                       sgx_node_batch_sample_quant writes for the same draw; a filler row holds fq_k(1) on its first entry
 *                       and fq_k(0) on its dealt spare entries, formed in the pad launch by the same device function;
 *   dead_row_q[k][r]  = row r holds no values_q[k] > 0, for every r < N;
 *   values_lean[k][e] (optional, NULL = not written) = values_norm[e] on the rows with dead_row_q[k], values_q[k][e]
 *                       elsewhere, for every e < C_a.
 * values_q / values_lean hold C_a floats, dead_row_q N bytes.  q is const: has_dead_rows_q is NOT written, the call reads
 * nothing back (a caller takes "some row may be dead" as a constant fact with the exact mask, as for dead_row).
 * Capturable, no allocation, no synchronisation, the same bits on every run.  With a set status every row is a filler
 * row in these arrays too.
 * The call requires, for every k, fq_k(1) > 0 and fq_k(0) == 0, evaluated on the host by the same rule.  Then no filler
 * row is dead under the quantised mask `values_q > 0` (its first entry is fq_k(1) > 0; its values_lean are its values_q),
 * and a filler row's spare entries carry no weight in the GCN aggregate (they are 0), so every consequence above holds for
 * the quantised adjacency as well: a filler row's D is 0 in every layer and it passes nothing on.  Both conditions hold for
 * the constants the reference publishes for w_qbits = 8, 4, 2, 1: zero_adj = 0 there, and round(inv_scale_adj) is 255, 15,
 * 30, 10 before the clip to the grid.  A live row may still be dead under the quantised mask alone (an entry may round to
 * 0); it then takes the inherited uniform softmax over all N columns.
 * Argument errors of the quantised call, before anything is launched: b, pad or q NULL: SGX_ERR_NULL; then those of
 * sgx_node_batch_sample_quant's quantiser arguments (b->dtype other than SGX_F32: SGX_ERR_UNSUPPORTED; n_sets outside
 * {1, 2} or qbits outside {8, 4, 2, 1}: SGX_ERR_SHAPE; values_q[k] or dead_row_q[k] NULL for a k < n_sets: SGX_ERR_NULL);
 * fq_k(1) <= 0 (or not a number) or fq_k(0) != 0 for some k -- the filler rows would be dead or would carry weight --:
 * SGX_ERR_UNSUPPORTED; then those of sgx_node_batch_sample_padded.
 *
 * Argument errors, before anything is launched: those of sgx_node_batch_sample (without its host outputs); b, pad or a
 * pointer of pad NULL: SGX_ERR_NULL; batch == 0, capacities below the rule's (N < mn, E < me, C_a < me + N, C_a - N >
 * 63 (N - mn), C_f > 64 (N - mn)) or over INT32_MAX: SGX_ERR_SHAPE; a fan-out of -1 (an unbounded row):
 * SGX_ERR_UNSUPPORTED.  sgx_node_batch_pad_capacity: pad or fanouts NULL: SGX_ERR_NULL; arguments the bounds refuse,
 * batch == 0, a negative row count or a capacity over INT32_MAX: SGX_ERR_SHAPE; a fan-out of -1: SGX_ERR_UNSUPPORTED. */
typedef struct sgx_node_batch_pad {
    int32_t n_rows;                            /* N */
    int32_t reserved;
    int64_t nnz_norm, nnz_fea, n_edges;        /* C_a, C_f, E */
    const uint64_t *step;                      /* device */
    int32_t *status;                           /* device, OR-ed into */
    int32_t *counts;                           /* device out [4 + 2 (n_hops + 1)] */
} sgx_node_batch_pad;

/* fills n_rows, nnz_norm, nnz_fea and n_edges of *pad by the rule; the pointers are left alone */
int sgx_node_batch_pad_capacity(int n_nodes, int64_t nnz, int batch, int n_hops, const int *fanouts,
                                const int32_t *fea_row_counts, sgx_node_batch_pad *pad);
int sgx_node_batch_sample_padded(sgx_node_batch *b, const sgx_node_batch_pad *pad, void *stream);
int sgx_node_batch_sample_padded_quant(sgx_node_batch *b, const sgx_node_batch_pad *pad, const sgx_node_batch_quant *q,
                                       void *stream);

/* ---- the node evaluation head: hits and the summed loss of a pass over node batches, kept on the device ----------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_node_eval is the evaluation of GAT_PYNQ behind the last layer -- Linear [C][P], arg-max against the label,
 * CrossEntropyLoss(reduction = sum) over out[mask] / out[:batch_size] -- for one batch of a pass over a loader
 * (demo_sgrace.py's test(loader, split)).  It is sgx_head_eval for the rows sgx_node_loss selects: it ADDS to accumulators
 * the caller zeroes once per pass, so batches of unequal size accumulate on the device and a pass is read back once.
 * H [n_rows][P], W [C][P], bias [C] or NULL fp32, target int64 [n_rows], mask bytes [n_rows] or NULL, all on the device.
 *   selection  sgx_node_loss's: row i is selected iff i < n_prefix && (mask == NULL || mask[i] != 0); M = their number,
 *              counted on the device (integers); the host never learns it.  n_prefix > n_rows selects as n_rows does.
 *   logits     z[i][c] of sgx_node_loss with p_drop = 0, bit for bit (x == H): one fmaf chain from 0 over j ascending from
 *              0 of W[c][j] * H[i][j], then + bias[c] (0 without a bias).  Not sgx_head_eval's 64-lane form.
 *   per selected row:  sgx_node_loss's per-row term, bit for bit: m = max_c z_c;  lse = m + logf(sum_c expf(z_c - m)),
 *              c ascending from 0;  loss_i = lse - z[target_i]
 *              hit_i: arg-max of z[i] == target_i, sgx_node_loss's arg-max: over c ascending with a strict > from z[0]
 *              (a NaN z[0] counts as -inf): the lowest index wins a tie, a NaN never wins
 *              a target outside [0, C): loss_i = 0, no hit, nothing is indexed; the row still counts in totals[0]
 *   the call adds:  totals[0] += M;  totals[1] += sum_i hit_i   (integers);
 *              loss_sum[0] += S, a double formed in two levels over blocks of SGX_NODE_LOSS_ROWS consecutive rows:
 *              s_b = (double)loss_i added from 0.0 over the selected rows i of block b in ascending row order;
 *              S = s_0 + s_1 + ... added from 0.0 over the blocks b = 0 .. ceil(min(n_prefix, n_rows) / SGX_NODE_LOSS_ROWS)
 *              - 1 in ascending block order (a block without a selected row adds 0.0); S is added to loss_sum[0] once.
 *              A full-graph call thus ends in n_rows / SGX_NODE_LOSS_ROWS sequential additions, not n_rows.
 *   M == 0     nothing is added: the accumulators keep their bits; only `logits` is written.
 *   unselected rows are never read for a sum (they may hold anything, NaN included); without `logits` a block of
 *              SGX_NODE_LOSS_ROWS rows without a selected row is not read at all, and an unselected row of another block is
 *              not read either.  logits, when given, receives z for every i < n_rows, selected or not.
 * Two launches, as sgx_head_eval: sgx_node_loss's walk without its gradients (W in LDS, a thread per (row, class)), every
 * block's record (s_b, its selected rows, its hits) to a slot of its own in the workspace, so nothing that is summed
 * depends on the grid; then one workgroup adds the records in block order and adds to the accumulators.  No atomics: the
 * same bits on every run, for any grid and on every device.  Capturable: no allocation, no synchronisation.  The
 * accumulators are read and written by the second launch, on the stream.
 *
 * Limits: sgx_node_loss's, P <= 1024, C <= 64, C * P <= 16384; beyond: SGX_ERR_UNSUPPORTED and a workspace size of 0.
 * Argument errors, returned before anything reaches the device, in this order: n_rows, P or C below 1, n_prefix < 0:
 * SGX_ERR_SHAPE; H, W, target, totals or loss_sum NULL: SGX_ERR_NULL (bias NULL: no bias; mask NULL: the prefix alone;
 * logits NULL: not written); over a limit: SGX_ERR_UNSUPPORTED; workspace missing or below
 * sgx_node_eval_workspace_bytes: SGX_ERR_WORKSPACE; not 256-byte aligned: SGX_ERR_ALIGN. */
/* 256 + 16 bytes per block of SGX_NODE_LOSS_ROWS rows among the first min(n_prefix, n_rows) (n_prefix < 0 as 0) rounded up
 * to 256 bytes; 0 for a shape the call refuses */
size_t sgx_node_eval_workspace_bytes(int64_t n_rows, int64_t n_prefix, int P, int C);
int sgx_node_eval(int64_t n_rows, int64_t n_prefix, int P, int C, const float *H, const float *W, const float *bias,
                  const int64_t *target, const uint8_t *mask, int64_t *totals /* [2] */, double *loss_sum /* [1] */,
                  float *logits /* or NULL */, void *workspace, size_t workspace_bytes, void *stream);

/* ---- model selection: keep the best epoch's weights on the device --------------------------------------
 * Added without a version bump (SGX_VERSION stays 110): every declaration below is new, and nothing above changes.
 *
 * sgx_keep_best is the reference training loop's `if test_acc > best_acc: torch.save(model.state_dict())`
 * (demo_sgrace.py:583-610) without the read-back: one call per epoch compares the counts an evaluation pass left in its
 * accumulators (sgx_head_eval / sgx_node_eval: int64 [3] = rows, hits, the bits of the double loss sum) with the best so
 * far, in integers, copies up to SGX_BEST_MAX_TENSORS fp32 tensors into a snapshot where the epoch wins, and appends the
 * epoch's sums to a log on the device, so a whole run is read back once.  The tensor table travels in the kernel
 * arguments, as sgx_adam_step's does.
 *   state      device int64 [4] = (best_n, best_hits, best_epoch, epoch); a fresh one is (1, 0, -1, 0): the fraction 0 / 1
 *              stands for the reference's best_acc = 0
 *   operands   (n, hits) = sums[0][0], sums[0][1] -- sums[0] is the pass that decides -- and e = state[3]
 *   better     exactly when  0 < n < 2^31  and  0 <= hits <= n  and  best_n < 2^31  and
 *                  hits * best_n > best_hits * n       (64-bit integers: no division, no floating point)
 *              the reference's strict >: an epoch that ties the best (1/3 after 2/6, the same counts again) does not
 *              replace it, an epoch without a hit never becomes best, and a candidate outside the bounds is not better
 *   where better:  dst[i] = src[i] bit for bit, i < n, for every tensor (n == 0: skipped); then
 *              best_n, best_hits, best_epoch = n, hits, e
 *   in every call, better or not:  with log != NULL and 0 <= e < log_rows, row e of the log [log_rows][3 * n_sums]
 *              receives the three words of sums[0], sums[1], ... in order (the loss sum's double as its 64 bits); then
 *              epoch = e + 1
 * Two launches, as sgx_adam_step: one copies and logs and only READS state, so every workgroup forms the same decision
 * from the same words; a trailing one-thread launch forms it once more and writes state.  No atomics.  The copy strides
 * the grid over every tensor: 16-byte stores over the 16-byte-aligned body of dst and single elements at both ends; a src
 * that is not aligned as its dst is read by dwords.  src and dst of one tensor must not overlap.
 *
 * Capturable: no allocation, no synchronisation, the same bits on every run.  Argument errors, returned before anything
 * reaches the device: d, state or one of sums[0 .. n_sums) NULL, src or dst NULL with n > 0, log NULL with log_rows > 0:
 * SGX_ERR_NULL; n_tensors outside 0 .. SGX_BEST_MAX_TENSORS, n_sums outside 1 .. SGX_BEST_MAX_SUMS, n < 0, log_rows < 0:
 * SGX_ERR_SHAPE; src == dst on a tensor with n > 0: SGX_ERR_UNSUPPORTED; a src or dst of such a tensor off a 4-byte
 * boundary: SGX_ERR_ALIGN. */
#define SGX_BEST_MAX_TENSORS 16
#define SGX_BEST_MAX_SUMS 4

typedef struct sgx_best_tensor {
    const float *src;            /* [n] fp32: the parameter */
    float *dst;                  /* [n] fp32: its snapshot */
    int64_t n;                   /* elements; 0 = skipped */
} sgx_best_tensor;

typedef struct sgx_best_desc {
    int32_t n_tensors;           /* 0 .. SGX_BEST_MAX_TENSORS */
    int32_t n_sums;              /* 1 .. SGX_BEST_MAX_SUMS; sums[0] is the one that decides */
    const int64_t *sums[SGX_BEST_MAX_SUMS];  /* device, each int64 [3] = (n, hits, loss_sum bits) */
    int64_t *state;              /* device int64 [4]: best_n, best_hits, best_epoch, epoch */
    int64_t *log;                /* device int64 [log_rows][3 * n_sums], or NULL */
    int64_t log_rows;
    sgx_best_tensor tensor[SGX_BEST_MAX_TENSORS];
} sgx_best_desc;

int sgx_keep_best(const sgx_best_desc *d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGX_H */
