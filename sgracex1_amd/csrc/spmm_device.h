// What the two aggregation files share (spmm_csr.hip: rows under a plan's schedule; spmm_flat.hip: stored entries cut into
// chunks): how a call's table decides the lane split, the gather-and-accumulate walk over a run of entries, and the row
// store.  Kernels, grids and the ownership of rows are each file's own.
#pragma once
#include "sgx_device.h"

// Tuning knobs (defaults = the measured best, tools/sweep_spmm.py):
#ifndef SGX_SPMM_NT_STORE
#define SGX_SPMM_NT_STORE 0          // non-temporal stores of D
#endif
#ifndef SGX_SPMM_ADJ_STYLE
#define SGX_SPMM_ADJ_STYLE 0   // A.H: gather + accumulate edge by edge (rolling window of loads)
#endif
#ifndef SGX_SPMM_FEA_STYLE
#define SGX_SPMM_FEA_STYLE 1   // X.W: all gathers of a step, then the arithmetic
#endif
#ifndef SGX_SPMM_PIECES
#define SGX_SPMM_PIECES 1            // pieces of LPR edges per loop iteration (gathers in flight x PIECES)
#endif

// The lane split of one call.  16-byte gathers need rows that start on a dword: buffer loads take dword-aligned addresses
// (gfx950 runs in unaligned-access mode) and are range-checked dword by dword, so a chunk that runs past the end of a row
// reads the neighbouring row's first elements into lanes that are never stored, and past the end of the table zeros.
// Rows on odd halves (P_w = 41 unpadded) would pair their last element with a dword outside the table, and the 64-bit
// pointer path (big) has no range check: those keep one element per lane unless rows are 16-byte aligned.
// slots = lanes x 16-byte chunks (vec) or lanes (one element each) that cover a row, a power of two up to 64.
struct sgx_lane_split {
    bool vec;
    int slots;
};
static inline sgx_lane_split sgx_spmm_lane_split(int dtype, const void *H, int64_t ldh, int n_feat, bool big)
{
    const size_t es = sgx_elem_size(dtype);
    const int per16 = (int)(16 / es);
    const bool rows16 = ((uintptr_t)H % 16 == 0) && ((ldh * es) % 16 == 0);
    const bool rows4 = !big && ((uintptr_t)H % 4 == 0) && ((ldh * es) % 4 == 0);
    sgx_lane_split s;
    s.vec = rows16 || rows4;
    s.slots = sgx_next_pow2(s.vec ? (n_feat + per16 - 1) / per16 : n_feat);
    if (s.slots > 64) s.slots = 64;
    return s;
}

namespace {

// Sum of  values[e] * H[columnIndex[e]][this lane's columns]  over e in [e0, e1) stepping `stride`
// edges between this group's LPR-edge pieces.  A lane owns CPL chunks of VEC consecutive columns
// (CPL x 16 bytes of the row); chunk_off[j] = byte offset of chunk j inside a row of H, or kOOB when
// that chunk lies beyond n_feat.
//   LPR x CPL x 16 bytes = one row of H.  CPL = 1 spends all lanes of a group on the row (8 edges per
//   step at F = 64 fp16); CPL = 2 / 4 halves / quarters the group, so a wavefront keeps 2x / 4x as
//   many rows in flight and wastes fewer gather slots on short rows -- chosen from the matrix's mean
//   degree (sgx_plan).  Gathers in flight per lane stay at 8 either way.
// BIG = the table is 4 GiB or larger: buffer offsets are 32 bit, so the gathers become 64-bit
// global loads under a per-edge predicate (the all-gathered H of an 8-GPU run crosses this size).
template <typename T, int VEC, int LPR, int CPL, bool BIG, int STYLE>
__device__ __forceinline__ void accumulate_edges(float *acc, int e0, int e1, int stride, int sub,
                                                 const int32_t *__restrict__ col, const T *__restrict__ val,
                                                 __amdgpu_buffer_rsrc_t rsrc, const T *__restrict__ table,
                                                 unsigned ld_bytes, const unsigned *chunk_off)
{
    // PIECES pieces of LPR edges are handled per iteration: their (column, value) pairs arrive with
    // one load each (requested one iteration ahead) and all their gathers are issued before the first
    // is consumed -- SGX_SPMM_PIECES * min(LPR, 8/CPL) * CPL gathers in flight per lane.
    constexpr int PIECES = SGX_SPMM_PIECES;
    // What travels from the lane that loaded an edge to the lanes that gather for it: the byte offset
    // of the neighbour's row (column index x row pitch, multiplied once by the loading lane instead
    // of once per receiving lane) -- kOOBRow for an edge past the end of the row, which makes every
    // gather of that slot an out-of-range buffer access (returns 0, no memory traffic) without any
    // per-gather predicate.  Tables of 4 GiB and more (BIG) keep the column index and a predicate.
    // (the prefetched column index stays raw until the iteration that uses it: multiplying at fetch time
    // would put the wait for the load right behind the load)
    unsigned c_next[PIECES];
    T a_next[PIECES];
    constexpr unsigned kNoEdge = 0xFFFFFFFFu;
    auto fetch = [&](int idx, unsigned &c, T &a) {
        // a slot past the end of the row: the sentinel wherever a predicate reads it (STYLE 1, and every style on the
        // 64-bit pointer path, which has no range check: column 0 would be loaded and 0 x inf = NaN)
        c = (STYLE == 0 && !BIG) ? 0u : kNoEdge;
        a = (T)0;
        if (idx < e1) {
            c = (unsigned)__builtin_nontemporal_load(col + idx);                 // streamed once: keep L2 for H
            a = __builtin_nontemporal_load(val + idx);
        }
    };
#pragma unroll
    for (int p = 0; p < PIECES; ++p) fetch(e0 + p * stride + sub, c_next[p], a_next[p]);
    for (int base = e0; base < e1; base += PIECES * stride) {
        unsigned r[PIECES];
        float a[PIECES];
#pragma unroll
        for (int p = 0; p < PIECES; ++p) {
            r[p] = (BIG || STYLE == 0) ? c_next[p] : (c_next[p] == kNoEdge ? kOOBRow : c_next[p] * ld_bytes);
            a[p] = Elem<T>::to_f32(a_next[p]);
            // the next iteration's (column, value) pairs are requested before this iteration's gathers
            fetch(base + (PIECES + p) * stride + sub, c_next[p], a_next[p]);
        }
#ifndef SGX_SPMM_ADJ_INFLIGHT
#define SGX_SPMM_ADJ_INFLIGHT 8
#endif
#ifndef SGX_SPMM_FEA_INFLIGHT
#define SGX_SPMM_FEA_INFLIGHT 4
#endif
        // edges of one piece whose gathers go together (the loop leaves a piece after the last group that
        // holds a valid edge, so a smaller group wastes fewer slots on short rows)
        constexpr int kInFlight = (STYLE == 1 ? SGX_SPMM_FEA_INFLIGHT : SGX_SPMM_ADJ_INFLIGHT) / CPL;
        static_assert(kInFlight >= 1, "SGX_SPMM_*_INFLIGHT must be at least the largest CPL (4): a group of 0 edges never advances");
        constexpr int UNR = LPR < kInFlight ? LPR : kInFlight;
#pragma unroll 1
        for (int t0 = 0; t0 < LPR; t0 += UNR) {
            if (t0 >= e1 - base) break;
            if constexpr (!BIG && STYLE == 0) {
                // gather and accumulate edge by edge; the compiler's schedule keeps a rolling window of
                // loads in flight across steps (best for the HBM-bound A.H stage)
#pragma unroll
                for (int p = 0; p < PIECES; ++p) {
                    const int n = e1 - base - p * stride;            // valid edges in this piece (may be <= 0)
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        // here the column index itself travels and every receiving lane forms its offset
                        // (measured: the A.H stage loses 1 % with the pre-multiplied row offset of STYLE 1)
                        const int t = t0 + u;
                        const unsigned cc = (unsigned)__shfl((int)r[p], t, LPR);
                        const float aa = __shfl(a[p], t, LPR);
#pragma unroll
                        for (int j = 0; j < CPL; ++j)
                            Gather<T, VEC>::run(acc + j * VEC, aa, rsrc,
                                                (t < n && chunk_off[j] != kOOB) ? cc * ld_bytes + chunk_off[j] : kOOB);
                    }
                }
            } else if constexpr (!BIG) {
                // all gathers of the step first, then the arithmetic (fewer registers, more wavefronts: best
                // for X.W, whose table sits in L2 and whose cost is instruction issue)
                typename GatherRaw<T, VEC>::raw_t raw[PIECES][UNR][CPL];
                float aa[PIECES][UNR];
#pragma unroll
                for (int p = 0; p < PIECES; ++p)
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const unsigned rr = (unsigned)__shfl((int)r[p], t0 + u, LPR);
                        aa[p][u] = __shfl(a[p], t0 + u, LPR);
#pragma unroll
                        for (int j = 0; j < CPL; ++j)       // a lane whose chunk lies beyond n_feat stays out of range
                            raw[p][u][j] = GatherRaw<T, VEC>::load(rsrc, chunk_off[j] != kOOB ? rr + chunk_off[j] : kOOB);
                    }
#pragma unroll
                for (int p = 0; p < PIECES; ++p)
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
#pragma unroll
                        for (int j = 0; j < CPL; ++j) GatherRaw<T, VEC>::fma(acc + j * VEC, aa[p][u], raw[p][u][j]);
            } else {
#pragma unroll
                for (int p = 0; p < PIECES; ++p)
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const unsigned rr = (unsigned)__shfl((int)r[p], t0 + u, LPR);
                        const float aa = __shfl(a[p], t0 + u, LPR);
#pragma unroll
                        for (int j = 0; j < CPL; ++j)
                            if (rr != 0xFFFFFFFFu && chunk_off[j] != kOOB)
                                GatherPtr<T, VEC>::run(acc + j * VEC, aa, reinterpret_cast<const char *>(table) +
                                                                              (size_t)rr * ld_bytes + chunk_off[j]);
                    }
            }
        }
    }
}

template <typename T, int VEC>
__device__ __forceinline__ void store_row(T *__restrict__ drow, int col0, int n_feat, const float *acc, int relu, const sgx_epilogue &ep)
{
    store_lane_outputs<T, VEC, SGX_SPMM_NT_STORE ? SGX_STORE_ELEM_ALIGNED_NT : SGX_STORE_ELEM_ALIGNED>(
        drow, col0, n_feat, true, [&](int i) SGX_LAMBDA_INLINE { return finish_value<T>(acc[i], relu, ep); });
}

}  // namespace
