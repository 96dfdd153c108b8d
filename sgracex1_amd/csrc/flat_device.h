// The entry-split ownership rule ("entry-split aggregation", include/sgx.h; in numpy: tests/_spmm_flat_ref.py), stated once
// for the forms that cut their work by stored entries: spmm_flat.hip (plain sums) and gat_flat.hip (edge softmax).
//   * the stored entries are cut into chunks of T = kFlatChunk consecutive entries, a wavefront per chunk.  Chunk c owns
//     the rows that START in [cT, (c+1)T) -- found by two searches in rowPtr, 64 probes a step -- and, where entry cT lies
//     inside a row that started earlier, that row's piece [cT, ...) (its head piece);
//   * a row wholly inside the chunk is finished by it;
//   * a row that crosses a chunk end leaves one partial per chunk it touches: the chunk it starts in (its leader) in that
//     chunk's tail slot (2c + 1), every later chunk k in its head slot (2k).  The leader also writes down the row and the
//     last chunk it reaches (meta[c]) for the second launch;
//   * an empty row starts at entry rowPtr[r] like any other and belongs to the chunk that owns that entry -- to the last
//     live chunk when the index is the matrix's end, to chunk 0 when the matrix holds nothing;
//   * the host's entry count may be a capacity: a chunk at or past rowPtr[n_rows] returns at once.
// spmm_flat.hip takes T, the piece kinds, the chunk count and the search from here and keeps its own text of
// flat_chunk_find / flat_piece inside its kernel: through these two functions its assembly was no longer the parent's
// (DESIGN 4.36).  A change to the rule is made in both places.
#pragma once
#include "sgx_device.h"

namespace {

constexpr int kFlatChunk = 256;      // T: 32 steps of a lane group at F = 64 fp16, 4 steps of the wavefront on one long row
constexpr int kFlatCoop = 64;        // a piece this long is taken by all lane groups together
constexpr int64_t kFlatMaxNnz = 0x7FFFFFFF;

enum { FLAT_NONE = 0, FLAT_ROW = 1, FLAT_HEAD = 2, FLAT_TAIL = 3 };

static inline int64_t flat_chunks(int64_t nnz) { return nnz <= 0 ? 1 : (nnz + kFlatChunk - 1) / kFlatChunk; }
static inline int flat_ldp(int n_feat) { return (int)sgx_align_up((size_t)n_feat, 4); }

// The first r in [0, n] with rowptr[r] >= x (n: none of rowptr[0, n) is), by the whole wavefront: lane l probes the last
// element of the l-th of 64 equal blocks of the range, so a step narrows it 64-fold -- 3 dependent loads for 2^18 rows
// where a bisection makes 18.  Reads rowptr[0, n) only, whatever the array holds.
__device__ __forceinline__ int wave_lower_bound(const int32_t *__restrict__ rowptr, int n, int x)
{
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = n;                           // the answer lies in [lo, hi]
    while (lo < hi) {
        const int step = (hi - lo - 1) / 64 + 1;
        const int64_t p = (int64_t)lo + (int64_t)(lane + 1) * step - 1;
        const bool ge = p >= hi || rowptr[p] >= x;
        const unsigned long long m = __ballot(ge);
        if (m == 0) return hi;                    // lane 63 probed hi - 1 and it is below x
        const int f = __ffsll(m) - 1;
        const int64_t pf = (int64_t)lo + (int64_t)(f + 1) * step - 1;
        lo += f * step;
        hi = pf < hi ? (int)pf : hi;
    }
    return lo;
}

// What chunk c of a wavefront owns: entries [lo, hi), the rows [r_a, r_b) that start there, the head piece [lo, head_end)
// of row r_a - 1 (has_head), and the row it leads (tail_row, or -1) with the last chunk that row reaches.
struct flat_chunk {
    int lo, hi, r_a, r_b, head_end, tail_row, tail_last;
    bool has_head;
};

// false: a chunk of the capacity behind the matrix's end, which owns nothing.  The leader facts go to meta[c] here, by lane
// 0, for every live chunk -- so the scratch needs no clearing.
__device__ __forceinline__ bool flat_chunk_find(flat_chunk &k, int c, int n_rows, int nnz_cap, int n_chunks,
                                                const int32_t *__restrict__ rowptr, int32_t *__restrict__ meta)
{
    // the matrix's own end, read here: nnz_cap is a bound on it (and what the arrays hold, so never read past it)
    int nnz = rowptr[n_rows];
    nnz = nnz < 0 ? 0 : (nnz > nnz_cap ? nnz_cap : nnz);
    const int64_t lo64 = (int64_t)c * kFlatChunk;
    if (lo64 >= nnz && !(c == 0 && nnz == 0)) return false;        // a chunk of the capacity behind the end
    const int lo = (int)lo64;
    const bool last = lo64 + kFlatChunk >= nnz;
    const int hi = last ? nnz : lo + kFlatChunk;

    const int lane = threadIdx.x & 63;
    const int r_a = wave_lower_bound(rowptr, n_rows, lo);                        // the rows that start here: [r_a, r_b)
    const int r_b = last ? n_rows : wave_lower_bound(rowptr, n_rows, hi);
    const int head_end = rowptr[r_a];                                            // (r_a <= n_rows)
    const bool has_head = r_a > 0 && head_end > lo && hi > lo;                   // entry lo lies in row r_a - 1
    int tail_row = -1, tail_last = 0;
    if (!last && r_b > r_a) {
        int e = rowptr[r_b];
        e = e > nnz ? nnz : e;
        if (e > hi) { tail_row = r_b - 1; tail_last = (e - 1) / kFlatChunk; }
    }
    if (lane == 0) {
        meta[2 * (int64_t)c] = tail_row;
        meta[2 * (int64_t)c + 1] = tail_last < n_chunks ? tail_last : n_chunks - 1;
    }
    k.lo = lo; k.hi = hi; k.r_a = r_a; k.r_b = r_b; k.head_end = head_end; k.tail_row = tail_row; k.tail_last = tail_last;
    k.has_head = has_head;
    return true;
}

// piece 0 = the head piece (or nothing), piece i >= 1 = row r_a + i - 1
__device__ __forceinline__ int64_t flat_pieces(const flat_chunk &k) { return 1 + (int64_t)(k.r_b - k.r_a); }

// Piece i of the chunk (any i; FLAT_NONE past the last): its kind, its row and its entries [e0, e1) inside the chunk.
__device__ __forceinline__ void flat_piece(const flat_chunk &k, int64_t i, int64_t n_pieces, const int32_t *__restrict__ rowptr,
                                           int &kind, int &r, int &e0, int &e1)
{
    kind = FLAT_NONE; r = 0; e0 = 0; e1 = 0;
    if (i == 0) {
        if (k.has_head) { kind = FLAT_HEAD; r = k.r_a - 1; e0 = k.lo; e1 = k.head_end; }
    } else if (i < n_pieces) {
        r = k.r_a + (int)(i - 1);
        kind = r == k.tail_row ? FLAT_TAIL : FLAT_ROW;
        e0 = rowptr[r];
        e1 = rowptr[r + 1];
    }
    // (a rowPtr that is not monotone must not send a read outside the chunk)
    e0 = e0 < k.lo ? k.lo : e0;
    e1 = e1 > k.hi ? k.hi : e1;
    e1 = e1 < e0 ? e0 : e1;
}

}  // namespace
