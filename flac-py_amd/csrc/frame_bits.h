/* frame_bits.h — what a unit is written as and how many bits that takes: the size functions the
 * frame writer (k_frame.hip) and the stereo chooser (k_stereo.hip) share, and the unit layout
 * of the stereo mode.  Device code only. */
#pragma once
#include "device_common.h"

namespace flacmi {

__device__ __forceinline__ int unit_len(const FrameArgs& a, int64_t u) {
    return u >= a.n_units - a.n_tail_units ? a.tail_len : a.block_len;
}

/* Bits of the subframe up to the first partition (encoder.py:553-627, :766-767).  ss: the width
 * the unit's samples are written at; w: its wasted bits (FLACMI_FRAME_WASTED: the header is
 * 0 tttttt 1, w - 1 zeros and a one, 8 + w bits, and ss is the stream's sample size less w). */
__device__ __forceinline__ uint32_t sub_prefix_bits(const flacmi_unit_meta& m, int ss, int q, int w = 0) {
    const bool lpc = m.kind == FLACMI_KIND_LPC;
    return 8u + (uint32_t)w + (uint32_t)m.order * (uint32_t)ss + (lpc ? 9u + (uint32_t)m.ncoefs * (uint32_t)q : 0u) + 6u;
}

/* Written residual bits (partition parameters + Rice codes) from the reference's estimate
 * rice_bits = sum_k [4 + (p_k > 14 ? 5 : 4) + data_k] (encoder.py:714-727):
 *   Rice4Bit: sum_k [4 + data_k]          = rice_bits - 4 n_parts
 *   Rice5Bit: sum_k [5 + data_k]          = rice_bits - 3 n_parts - #{p_k > 14} */
__device__ __forceinline__ int64_t sub_residual_bits(const flacmi_unit_meta& m, int cnt14) {
    return m.coding_method == 5 ? m.rice_bits - 3LL * m.n_parts - cnt14 : m.rice_bits - 4LL * m.n_parts;
}

/* What unit u is written as.  FB: the build of a kernel for the fallback mode (a.sub_kind
 * set); the builds for the mode off never look at the array, so they are the code they were
 * before the mode existed (an a.sub_kind test at run time cost k_packw2k 0.6% and
 * k_frame_sizes 5% on config 2's frames). */
template <bool FB>
__device__ __forceinline__ int sub_kind_of(const FrameArgs& a, int64_t u) {
    if constexpr (FB) return a.sub_kind[u];
    else return 0;
}

/* Bits of a CONSTANT / VERBATIM subframe (encoder.py:553-578): the header byte (and the w bits
 * of the wasted code) and one or n samples of ss bits. */
__device__ __forceinline__ uint32_t sub_raw_bits(int kind, int n, int ss, int w = 0) {
    return 8u + (uint32_t)w + (kind == FLACMI_SUB_CONSTANT ? 1u : (uint32_t)n) * (uint32_t)ss;
}

/* WB: the build of a kernel for the wasted-bits mode (a.wasted set; never together with ST); the
 * other builds never look at the array, so they are the code they were before the mode existed. */
template <bool WB>
__device__ __forceinline__ int unit_wasted(const FrameArgs& a, int64_t u) {
    if constexpr (WB) return a.wasted[u];
    else return 0;
}

/* ---- the stereo mode's units (FLACMI_STEREO_BEST, a.choice set) ------------------------
 * With F = a.n_frames the analysis outputs (meta, rice_params, residual rows, sub_kind) hold
 * 4 F candidate units: [0, 2F) the caller's rows (2f left, 2f + 1 right), [2F, 3F) the mid
 * rows (a.mid, the caller's element type) and [3F, 4F) the side rows (a.side, int32, one bit
 * wider than the stream's sample size).  a.n_units stays the caller's 2 F.  ST: the build of a
 * kernel for the mode; the other builds are the code they were before it existed. */
__device__ __forceinline__ int64_t st_frame_of(const FrameArgs& a, int64_t u) {
    const int64_t F = a.n_frames;
    return u < 2 * F ? u >> 1 : u < 3 * F ? u - 2 * F : u - 3 * F;
}

template <bool ST>
__device__ __forceinline__ int unit_len_of(const FrameArgs& a, int64_t u) {
    if constexpr (ST) return st_frame_of(a, u) == a.n_frames - 1 ? a.tail_len : a.block_len;
    else return unit_len(a, u);
}

/* bits of a warm-up or raw sample of unit u; w: the unit's wasted bits (unit_wasted) */
template <bool ST>
__device__ __forceinline__ int unit_bits_of(const FrameArgs& a, int64_t u, int w = 0) {
    if constexpr (ST) return a.sample_size + (u >= 3 * a.n_frames ? 1 : 0);
    else return a.sample_size - w;
}

/* unit u's sample row and its element size in bytes */
template <bool ST>
__device__ __forceinline__ const uint8_t* unit_row(const FrameArgs& a, int64_t u, int& sb) {
    if constexpr (ST) {
        const int64_t F = a.n_frames;
        if (u >= 3 * F) {
            sb = 4;
            return (const uint8_t*)(a.side + (u - 3 * F) * a.side_stride);
        }
        sb = a.sample_bytes;
        if (u >= 2 * F) return (const uint8_t*)a.mid + (u - 2 * F) * a.mid_stride * sb;
    } else {
        sb = a.sample_bytes;
    }
    return (const uint8_t*)a.samples + u * a.stride * sb;
}

/* sample i of unit u */
template <bool ST>
__device__ __forceinline__ int64_t unit_sample(const FrameArgs& a, int64_t u, int i) {
    if constexpr (ST) {
        int sb;
        const uint8_t* row = unit_row<true>(a, u, sb);
        return sb == 2 ? (int64_t)((const int16_t*)row)[i] : (int64_t)((const int32_t*)row)[i];
    } else {
        return a.sample_bytes == 2 ? (int64_t)((const int16_t*)a.samples)[u * a.stride + i]
                                   : (int64_t)((const int32_t*)a.samples)[u * a.stride + i];
    }
}

/* Exact bits of candidate unit u as the frame writer writes it, from its meta, its Rice
 * parameters (cnt14: how many exceed 14, counted by the caller when coding_method is 5) and, in
 * the fallback mode, its sub-kind.  Not for a unit that fails (callers test that first). */
template <bool FB, bool ST>
__device__ __forceinline__ int64_t unit_sub_bits(const FrameArgs& a, int64_t u, int cnt14) {
    const int w = unit_bits_of<ST>(a, u);
    if (const int kind = sub_kind_of<FB>(a, u)) return sub_raw_bits(kind, unit_len_of<ST>(a, u), w);
    const flacmi_unit_meta& m = a.meta[u];
    return (int64_t)sub_prefix_bits(m, w, a.q) + sub_residual_bits(m, cnt14);
}

}  // namespace flacmi
