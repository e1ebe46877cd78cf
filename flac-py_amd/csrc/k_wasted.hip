/* k_wasted.hip — wasted bits of every unit of a batch (flacmi_wasted_rows_device).
 *
 * A FLAC subframe may declare k "wasted bits": the k low bits that are zero in every sample of
 * the block; they are shifted out before prediction and shifted back in after decoding.  The
 * reference's SubframeHeader carries the field (common.py:309) and every one of its encoder paths
 * writes 0 (encoder.py:326, :556).  The rule (include/flacmi.h): with m the bitwise OR of the
 * unit's n samples in two's complement, w = 0 when m == 0 (digital silence has no wasted bits),
 * otherwise w = min(ctz(m), sample_bits - 1); the unit becomes x_i >> w (arithmetic, exact).
 *
 *   k_wasted_rows    one workgroup a unit, memory-bound, no scratch.  Pass 1 ORs the row (16-byte
 *                    loads, a wave reduce by shuffles, an LDS combine across the 4 waves) and
 *                    writes wasted[u]; pass 2 reads the row again (the workgroup has just read it:
 *                    it comes from L2) and stores x >> w.  In place a unit with w == 0 has no
 *                    pass 2, so a batch without wasted bits costs one read of its samples.
 */
#include "device_common.h"

namespace flacmi {

constexpr int kWastedThreads = 256; /* the launch's workgroup: the LDS combine below holds one word a wave */
static_assert(kWastedThreads % 64 == 0, "whole waves");

/* T: int16_t or int32_t rows.  A group is the G = 16 / sizeof(T) samples of one 16-byte load.  The
 * group the unit's length falls into is read and written sample by sample: nothing at or past the
 * length is read, enters the OR or is written, in place or not.  A thread shifts the groups it
 * ORed, and the barrier between the passes lies behind every load of pass 1, so out == in is safe. */
template <typename T>
__global__ __launch_bounds__(kWastedThreads) void k_wasted_rows(const T* in, int64_t in_stride, int64_t n_units,
                                                     int32_t block_len, int32_t tail_len, int64_t n_tail_units,
                                                     int32_t sample_bits, T* out, int64_t out_stride,
                                                     int32_t* __restrict__ wasted) {
    constexpr int G = 16 / (int)sizeof(T);
    union Vec {
        uint4 v;
        T e[G];
    };
    __shared__ uint32_t wave_or[kWastedThreads / 64];
    const int64_t u = blockIdx.x;
    const int n = u >= n_units - n_tail_units ? tail_len : block_len;
    const T* src = in + u * in_stride;
    T* dst = out + u * out_stride;
    const int groups = (n + G - 1) / G;

    uint32_t m = 0;
    for (int g = threadIdx.x; g < groups; g += kWastedThreads) {
        const int i0 = g * G;
        if (i0 + G <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + i0);
            m |= v.x | v.y | v.z | v.w; /* int16 rows: two samples a dword, folded below */
        } else {
            for (int i = i0; i < n; ++i) m |= sizeof(T) == 2 ? (uint32_t)(uint16_t)src[i] : (uint32_t)src[i];
        }
    }
    if (sizeof(T) == 2) m = (m | (m >> 16)) & 0xffffu; /* both halves of every dword onto 16 bits */
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m |= __shfl_xor(m, o);
    if ((threadIdx.x & 63) == 0) wave_or[threadIdx.x >> 6] = m;
    __syncthreads();
    m = 0;
#pragma unroll
    for (int k = 0; k < kWastedThreads / 64; ++k) m |= wave_or[k];
    int w = m == 0 ? 0 : __builtin_ctz(m);
    if (w > sample_bits - 1) w = sample_bits - 1;
    if (threadIdx.x == 0) wasted[u] = w;
    if (w == 0 && src == dst) return;

    for (int g = threadIdx.x; g < groups; g += kWastedThreads) {
        const int i0 = g * G;
        if (i0 + G <= n) {
            Vec x;
            x.v = *reinterpret_cast<const uint4*>(src + i0);
#pragma unroll
            for (int e = 0; e < G; ++e) x.e[e] = (T)(x.e[e] >> w);
            *reinterpret_cast<uint4*>(dst + i0) = x.v;
        } else {
            for (int i = i0; i < n; ++i) dst[i] = (T)(src[i] >> w);
        }
    }
}

hipError_t launch_wasted_rows(const void* in, int32_t sample_bytes, int64_t in_stride, int64_t n_units,
                              int32_t block_len, int32_t tail_len, int64_t n_tail_units, int32_t sample_bits,
                              void* out, int64_t out_stride, int32_t* wasted, hipStream_t s) {
    if (n_units <= 0) return hipSuccess;
    const dim3 g((unsigned)n_units), t(kWastedThreads);
    if (sample_bytes == 2)
        hipLaunchKernelGGL(k_wasted_rows<int16_t>, g, t, 0, s, (const int16_t*)in, in_stride, n_units, block_len,
                           tail_len, n_tail_units, sample_bits, (int16_t*)out, out_stride, wasted);
    else
        hipLaunchKernelGGL(k_wasted_rows<int32_t>, g, t, 0, s, (const int32_t*)in, in_stride, n_units, block_len,
                           tail_len, n_tail_units, sample_bits, (int32_t*)out, out_stride, wasted);
    return hipGetLastError();
}

}  // namespace flacmi
