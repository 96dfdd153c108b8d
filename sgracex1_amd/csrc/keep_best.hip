// Model selection on the device (sgx_keep_best, include/sgx.h "model selection"): the reference loop's
// `if test_acc > best_acc: torch.save(model.state_dict())` as one call per epoch.  The counts an evaluation pass left in
// its accumulators are compared with the best so far in 64-bit integers; where the epoch wins, up to SGX_BEST_MAX_TENSORS
// fp32 tensors are copied into their snapshots; in every call the epoch's sums go to a row of a device log.  The tensor
// table is passed by value in the kernel arguments (nothing is uploaded), and the state lives on the device -- so one
// captured call is the right decision at every replay.
//
// The first launch copies and logs and only reads the state: every workgroup forms the same decision from the same
// words, whatever the grid.  A trailing one-thread launch forms it once more and writes the state.  No atomics.
#include "sgx_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;       // 8 workgroups of 256 on each of 256 CUs; the copy strides over what is left

struct BestTable {
    sgx_best_tensor t[SGX_BEST_MAX_TENSORS];
    const int64_t *sums[SGX_BEST_MAX_SUMS];
    int32_t n, n_sums;                 // n: the tensors with n > 0
    int64_t *state, *log;
    int64_t log_rows;
};

struct alignas(16) Vec16 {
    uint32_t w[4];
};

// the rule of include/sgx.h, in one place for both launches
__device__ __forceinline__ bool better(int64_t n, int64_t hits, int64_t best_n, int64_t best_hits)
{
    constexpr int64_t kLimit = (int64_t)1 << 31;
    if (!(n > 0 && n < kLimit && hits >= 0 && hits <= n && best_n < kLimit)) return false;
    return hits * best_n > best_hits * n;
}

// dst[0 .. n) = src[0 .. n) as 32-bit words by threads t, t + nt, ...: 16-byte stores over the 16-byte-aligned body of
// dst, single words in front of and behind it; the body's loads are 16 bytes where src is aligned as dst is, else dwords
__device__ __forceinline__ void copy_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, int64_t n, int64_t t,
                                           int64_t nt)
{
    int64_t head = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15) / 4;
    if (head > n) head = n;
    const int64_t body = (n - head) / 4;
    if (t < head) dst[t] = src[t];
    Vec16 *__restrict__ d4 = reinterpret_cast<Vec16 *>(dst + head);
    const uint32_t *__restrict__ s = src + head;
    if (((uintptr_t)s & 15) == 0) {
        const Vec16 *__restrict__ s4 = reinterpret_cast<const Vec16 *>(s);
        for (int64_t i = t; i < body; i += nt) d4[i] = s4[i];
    } else {
        for (int64_t i = t; i < body; i += nt) {
            Vec16 v;
            v.w[0] = s[4 * i], v.w[1] = s[4 * i + 1], v.w[2] = s[4 * i + 2], v.w[3] = s[4 * i + 3];
            d4[i] = v;
        }
    }
    for (int64_t i = head + body * 4 + t; i < n; i += nt) dst[i] = src[i];
}

__global__ __launch_bounds__(kBlock) void keep_best_kernel(BestTable a)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x, nt = (int64_t)gridDim.x * kBlock;
    const int64_t e = a.state[3];
    if (a.log && e >= 0 && e < a.log_rows) {
        const int words = 3 * a.n_sums;
        for (int64_t i = t; i < words; i += nt) a.log[e * words + i] = a.sums[i / 3][i % 3];
    }
    if (!better(a.sums[0][0], a.sums[0][1], a.state[0], a.state[1])) return;
    for (int k = 0; k < a.n; ++k)
        copy_words(reinterpret_cast<uint32_t *>(a.t[k].dst), reinterpret_cast<const uint32_t *>(a.t[k].src), a.t[k].n, t, nt);
}

__global__ void keep_best_advance_kernel(const int64_t *sums, int64_t *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t n = sums[0], hits = sums[1], e = state[3];
    if (better(n, hits, state[0], state[1])) state[0] = n, state[1] = hits, state[2] = e;
    state[3] = e + 1;
}

}  // namespace

extern "C" int sgx_keep_best(const sgx_best_desc *d, void *stream)
{
    if (!d || !d->state) return SGX_ERR_NULL;
    if (d->n_tensors < 0 || d->n_tensors > SGX_BEST_MAX_TENSORS || d->n_sums < 1 || d->n_sums > SGX_BEST_MAX_SUMS)
        return SGX_ERR_SHAPE;
    for (int k = 0; k < d->n_sums; ++k)
        if (!d->sums[k]) return SGX_ERR_NULL;
    if (d->log_rows < 0) return SGX_ERR_SHAPE;
    if (!d->log && d->log_rows > 0) return SGX_ERR_NULL;
    BestTable a = {};
    int64_t vectors = 0;
    for (int k = 0; k < d->n_tensors; ++k) {
        const sgx_best_tensor &t = d->tensor[k];
        if (t.n < 0) return SGX_ERR_SHAPE;
        if (t.n == 0) continue;
        if (!t.src || !t.dst) return SGX_ERR_NULL;
        if (t.src == t.dst) return SGX_ERR_UNSUPPORTED;
        if (((uintptr_t)t.src | (uintptr_t)t.dst) & 3) return SGX_ERR_ALIGN;
        a.t[a.n++] = t;
        vectors += (t.n + 3) / 4;
    }
    for (int k = 0; k < d->n_sums; ++k) a.sums[k] = d->sums[k];
    a.n_sums = d->n_sums;
    a.state = d->state, a.log = d->log, a.log_rows = d->log ? d->log_rows : 0;
    int64_t blocks = (vectors + kBlock - 1) / kBlock;
    blocks = blocks < 1 ? 1 : blocks > kMaxBlocks ? kMaxBlocks : blocks;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(keep_best_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    SGX_LAUNCH_CHECK();
    hipLaunchKernelGGL(keep_best_advance_kernel, dim3(1), dim3(64), 0, s, d->sums[0], d->state);
    SGX_LAUNCH_CHECK();
    return SGX_OK;
}
