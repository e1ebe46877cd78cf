/* k_stereo.hip — stereo decorrelation for the device encoder (FLACMI_STEREO_BEST).
 *
 * The reference's encoder writes Channels.L_R for every frame (encoder.py:95); its decoder
 * undoes all four stereo assignments (decoder.py:111-122, :431-451).  The per-channel analysis
 * (encode_subframe_fixed, encode_subframe_lpc, encode_residual) never looks at the sample size,
 * so a mid or side signal is analysed exactly as a channel holding those samples would be.
 *
 *   k_stereo_rows    mid = (L + R) >> 1 in the input's element type and side = L - R in int32
 *                    (one bit wider than the input) for every frame's row pair.  Memory-bound:
 *                    one workgroup a frame, 16-byte loads and stores, no LDS.
 *   k_stereo_choose  one wave per frame, after the analysis of the 4 n_frames candidate units
 *                    (frame_bits.h) and, in the fallback mode, k_sub_kinds over all of them: the
 *                    exact subframe size of left, right, mid and side as the frame writer will
 *                    write them, then the first of L_R, L_S, S_R, M_S with the smallest sum among
 *                    the assignments whose two candidates can be written.
 */
#include "device_common.h"
#include "frame_bits.h"

namespace flacmi {

/* T: int16_t or int32_t rows.  A group is the G = 16 / sizeof(T) samples of one 16-byte load of
 * each input row; it gives one 16-byte store of mid and G / 4 of side.  Groups at and past the
 * row's length write zeros up to each output pitch; the group the length falls into is read
 * sample by sample (nothing past a row's length is read). */
template <typename T>
__global__ __launch_bounds__(256) void k_stereo_rows(const T* __restrict__ lr, int64_t lr_stride, int64_t n_frames,
                                                     int32_t block_len, int32_t tail_len, int32_t has_tail,
                                                     T* __restrict__ mid, int64_t mid_stride,
                                                     int32_t* __restrict__ side, int64_t side_stride) {
    constexpr int G = 16 / (int)sizeof(T);
    union Vec {
        uint4 v;
        T e[G];
    };
    const int64_t f = blockIdx.x;
    const int n = has_tail && f == n_frames - 1 ? tail_len : block_len;
    const T* __restrict__ L = lr + 2 * f * lr_stride;
    const T* __restrict__ R = L + lr_stride;
    T* __restrict__ M = mid + f * mid_stride;
    int32_t* __restrict__ S = side + f * side_stride;
    const int64_t pitch = mid_stride > side_stride ? mid_stride : side_stride;
    const int64_t groups = (pitch + G - 1) / G;
    for (int64_t g = threadIdx.x; g < groups; g += blockDim.x) {
        const int64_t i0 = g * G;
        Vec l, r, m;
        if (i0 + G <= n) {
            l.v = *reinterpret_cast<const uint4*>(L + i0);
            r.v = *reinterpret_cast<const uint4*>(R + i0);
        } else {
#pragma unroll
            for (int e = 0; e < G; ++e) {
                l.e[e] = i0 + e < n ? L[i0 + e] : (T)0;
                r.e[e] = i0 + e < n ? R[i0 + e] : (T)0;
            }
        }
        int32_t s[G];
#pragma unroll
        for (int e = 0; e < G; ++e) {
            const int32_t a = l.e[e], b = r.e[e];
            m.e[e] = (T)((a >> 1) + (b >> 1) + (a & b & 1)); /* floor((a + b) / 2) without the 33rd bit */
            s[e] = (int32_t)((uint32_t)a - (uint32_t)b);
        }
        if (i0 + G <= mid_stride) *reinterpret_cast<uint4*>(M + i0) = m.v;
#pragma unroll
        for (int k = 0; k < G; k += 4)
            if (i0 + k + 4 <= side_stride)
                *reinterpret_cast<int4*>(S + i0 + k) = int4{s[k], s[k + 1], s[k + 2], s[k + 3]};
    }
}

hipError_t launch_stereo_rows(const void* lr, int32_t sample_bytes, int64_t lr_stride, int64_t n_frames,
                              int32_t block_len, int32_t tail_len, int32_t has_tail, void* mid, int64_t mid_stride,
                              int32_t* side, int64_t side_stride, hipStream_t s) {
    if (n_frames <= 0) return hipSuccess;
    const dim3 g((unsigned)n_frames), t(256);
    if (sample_bytes == 2)
        hipLaunchKernelGGL(k_stereo_rows<int16_t>, g, t, 0, s, (const int16_t*)lr, lr_stride, n_frames, block_len,
                           tail_len, has_tail, (int16_t*)mid, mid_stride, side, side_stride);
    else
        hipLaunchKernelGGL(k_stereo_rows<int32_t>, g, t, 0, s, (const int32_t*)lr, lr_stride, n_frames, block_len,
                           tail_len, has_tail, (int32_t*)mid, mid_stride, side, side_stride);
    return hipGetLastError();
}

/* One wave per frame.  A candidate is not eligible when its unit fails (and, in the fallback
 * mode, is not escaped) or when it is an LPC subframe the writer's precision assertion
 * (encoder.py:619) would stop; FLACMI_STATUS_RESIDUAL_WIDE on any candidate fails the frame with
 * that status, so the caller's redo with 8-byte residual rows still happens.  With no eligible
 * assignment the choice is L_R, and k_frame_sizes gives the frame the status it has without the
 * mode. */
template <bool FB>
__device__ __forceinline__ void stereo_choose(const FrameArgs& a) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t F = a.n_frames;
    if (f >= F) return;
    const int64_t cand[4] = {2 * f, 2 * f + 1, 2 * F + f, 3 * F + f}; /* left, right, mid, side */
    int64_t size[4];
    bool ok[4];
    int wide = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t u = cand[k];
        const flacmi_unit_meta& m = a.meta[u];
        ok[k] = true;
        size[k] = 0;
        int cnt = 0;
        if (sub_kind_of<FB>(a, u) == 0) { /* an escaped unit's meta is not read */
            if (m.status != 0) {
                if (m.status == FLACMI_STATUS_RESIDUAL_WIDE && wide == 0) wide = (m.site << 16) | m.status;
                ok[k] = false;
                continue;
            }
            if (m.kind == FLACMI_KIND_LPC && ((a.q - 1) & 15) == 15) {
                ok[k] = false;
                continue;
            }
            if (m.coding_method == 5) {
                const int32_t* rp = a.rice_params + u * a.params_stride;
                for (int j = lane; j < m.n_parts; j += 64) cnt += rp[j] > 14 ? 1 : 0;
                for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
            }
        }
        size[k] = unit_sub_bits<FB, true>(a, u, cnt);
    }
    /* L_R, L_S, S_R, M_S in this order; the first smallest sum wins */
    constexpr int code[4] = {1, 8, 9, 10}, first[4] = {0, 0, 3, 2}, second[4] = {1, 3, 1, 3};
    StereoChoice c{code[0], wide, {cand[0], cand[1]}}; /* no eligible assignment, or a wide candidate: L_R */
    bool found = false;
    int64_t best_bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { /* unrolled: every index below is a constant, nothing goes to scratch */
        const int64_t bits = size[first[i]] + size[second[i]];
        if (wide == 0 && ok[first[i]] && ok[second[i]] && (!found || bits < best_bits)) {
            found = true;
            best_bits = bits;
            c.code = code[i];
            c.unit[0] = cand[first[i]];
            c.unit[1] = cand[second[i]];
        }
    }
    if (lane == 0) a.choice[f] = c;
}
__global__ __launch_bounds__(256) void k_stereo_choose(FrameArgs a) { stereo_choose<false>(a); }
__global__ __launch_bounds__(256) void k_stereo_choose_fb(FrameArgs a) { stereo_choose<true>(a); }

hipError_t launch_stereo_choose(const FrameArgs& a, hipStream_t s) {
    if (a.n_frames <= 0) return hipSuccess;
    const dim3 g((unsigned)((a.n_frames + 3) / 4)), t(256);
    if (a.sub_kind) hipLaunchKernelGGL(k_stereo_choose_fb, g, t, 0, s, a);
    else hipLaunchKernelGGL(k_stereo_choose, g, t, 0, s, a);
    return hipGetLastError();
}

}  // namespace flacmi
