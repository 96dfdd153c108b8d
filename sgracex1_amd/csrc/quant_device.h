// The fake quantiser of one fp32 value (SG.py:177-265), shared by every kernel that puts values on the w_qbits grid:
// quant.hip (sgx_fake_quantize) and node_batch.hip (the quantised adjacency of a prepared batch).  One statement of the
// rounding points, so that every caller gives the same bits.  Host code may evaluate it too (node_batch.hip checks the
// filler entries of a padded quantised batch with it): IEEE fp32, round to nearest even, as on the device.
#pragma once
#include <hip/hip_runtime.h>

namespace sgx_quantizer {

__host__ __device__ __forceinline__ float clipf(float v, float lo, float hi)
{
    // torch.clip: min(max(v, lo), hi); NaN propagates
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// kind 0: quantization_ufbits (SG.py:253-265): unsigned grid 0 .. 2^q - 1
// kind 1: quantization_fbits  (SG.py:238-251): signed grid -(2^(q-1) - 1) .. 2^(q-1) - 1
__host__ __device__ __forceinline__ float fake_quantize_value(int kind, int qbits, float inv_scale, float zero, float x)
{
// `1 / s * x + z` is a rounded product followed by a rounded sum in the reference (two torch ops), not one fma -- in
// whatever kernel this is inlined
#pragma clang fp contract(off)
    const float lo = kind ? -(float)((1 << (qbits - 1)) - 1) : 0.0f;
    const float hi = kind ? (float)((1 << (qbits - 1)) - 1) : (float)((1 << qbits) - 1);
    const float back = 1.0f / (float)(1 << (qbits - 1));          // x_q / 2^(w_qbits - 1), SG.py:220
    const float t = inv_scale * x + zero;                          // 1 / s * x + z
    if (qbits == 1 && kind == 1) return t < 0.0f ? -0.5f : 0.5f;   // fake_quantization_b, SG.py:177-182
    if (qbits == 1) return clipf(rintf(t), 0.0f, 1.0f) * 0.5f;     // fake_quantization_b2, SG.py:184-189
    return clipf(rintf(t), lo, hi) * back;                         // fake_quantization, SG.py:191-235
}

// Host: what every padded batch requires of an adjacency grid before it launches (include/sgx.h, "padded node batches" and
// "padded batches"): the filler rows' diagonal 1 stays positive -- a 1 that rounds to 0 would leave them dead under the
// quantised mask -- and their spare 0 stays 0 -- it would otherwise carry weight.  Not-a-number fails both.
inline bool filler_entries_stay_inert(int qbits, float inv_scale, float zero)
{
    return fake_quantize_value(0, qbits, inv_scale, zero, 1.0f) > 0.0f && fake_quantize_value(0, qbits, inv_scale, zero, 0.0f) == 0.0f;
}

}  // namespace sgx_quantizer
