// The long-row walk of the GAT backward, stated once for gat_bwd_long_rows_kernel (gat_bwd.hip, a window of 64 rows) and
// attention_grad_slices_kernel (layer_bwd.hip, 64, window after window over the workgroup's run of rows).  Rows of up to
// kLongRowCut entries are taken by a few lanes each in those files; a longer row is taken by a whole workgroup, which
// finds it here.  gat_row_stats_long_kernel (gat_stats.hip, a window of 8) keeps its own text of the walk: measured there.
#pragma once

constexpr int kLongRowCut = 256;         // rows over this many entries: the whole workgroup

// The window of SPAN (at most 64) consecutive rows from `first`, cut at `end`: the first wavefront ballots "more than CUT
// entries" into *mask, an LDS word of the caller's, and every thread of the workgroup then calls body(r) for each such
// row in ascending order -- uniformly, so the body may hold barriers.  The barrier at the head lets every thread read the
// word of the window before: a caller may loop over windows on one word.  Every thread of the workgroup must call it.
template <int SPAN, int CUT, typename Body>
__device__ __forceinline__ void for_each_long_row(const int32_t *__restrict__ rowptr, int64_t first, int64_t end,
                                                  unsigned long long *mask, Body &&body)
{
    static_assert(SPAN >= 1 && SPAN <= 64, "one ballot of the first wavefront");
    __syncthreads();
    if (threadIdx.x < 64) {
        const int64_t r = first + threadIdx.x;
        const int deg = ((int)threadIdx.x < SPAN && r < end) ? rowptr[r + 1] - rowptr[r] : 0;
        const unsigned long long m = __ballot(deg > CUT);
        if (threadIdx.x == 0) *mask = m;
    }
    __syncthreads();
    unsigned long long todo = *mask;
    while (todo) {
        const int64_t r = first + (__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        body(r);
    }
}
