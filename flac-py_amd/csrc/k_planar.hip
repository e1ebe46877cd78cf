/* k_planar.hip — the decoder's rows of many streams as one padded planar buffer
 * (flacmi_planar_out_device): sample t of channel c of stream s goes to
 * out[(s * C + c) * pitch + t], as int16 (range-checked), int32 or float32.
 *
 * The frame list is k_pcm's and k_units' (planar int32 rows, each frame with its own pitch,
 * first_sample and block_size), ordered by (stream, first_sample), the stream index in
 * flacmi_pcm_frame.reserved0; first_sample counts from the frame's own stream's first sample.
 *
 * A gather, as k_units: a workgroup owns kPlanarThreads 16-byte groups of one output row and
 * nothing else, so
 *   - whatever the frame list holds, no byte outside the N * C rows is written;
 *   - the zero fill from the stream's length to the pitch, and the whole row of a stream with
 *     no frame, is the same loop as the samples: every group of every row is stored once, whole;
 *   - a frame boundary may fall anywhere inside a group (192-sample blocks of int16 fall on a
 *     group edge, 4608 + 1 do not); a scatter, one workgroup per frame as k_pcm, would write
 *     such a group from two workgroups in parts, and would leave the tail of every row and the
 *     rows of empty streams to another kernel.
 * Rows here are short (a clip, not a 795 MB stream) and frames are shorter still, so a lane owns
 * one group: it finds the frame of its first element by a binary search over the frames that can
 * hold the workgroup's elements (found by two wave-uniform searches, scalar loads) and steps to
 * the next frame where its group runs over a frame's end.  The lanes of a wave read consecutive
 * 16 or 32 bytes of a source row each, and store 16 bytes each: 1 KiB per wave instruction.
 * No LDS, no scratch (the group's elements are registers: every loop over them is unrolled).
 *
 * Range check (int16 only): a sample read that does not fit 16 bits sets its frame's status
 * word (every finder writes the same value).  float32: one v_cvt_f32_i32 (round to nearest
 * even) and the exact scale 2^-(sample_size - 1). */
#include "flacmi_kernels.h"

namespace flacmi {

constexpr int kPlanarThreads = 256; /* 16-byte groups of a row per workgroup */

/* the largest f in [lo, hi) whose (stream, first_sample) <= (s, t), or lo - 1 */
__device__ __forceinline__ int64_t planar_frame_at(const flacmi_pcm_frame* __restrict__ fr, int64_t lo, int64_t hi,
                                                   int32_t s, int64_t t) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int32_t ms = fr[mid].reserved0;
        if (ms < s || (ms == s && fr[mid].first_sample <= t)) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

/* ELEM: flacmi_planar_elem */
template <typename T, int ELEM>
__global__ __launch_bounds__(kPlanarThreads) void k_planar(PlanarArgs a) {
    constexpr int G = 16 / (int)sizeof(T);
    const int64_t row = blockIdx.x / a.tiles;
    const int64_t tile = blockIdx.x - row * a.tiles;
    const int32_t s = (int32_t)(row / a.channels);
    const int c = (int)(row - (int64_t)s * a.channels);
    const flacmi_pcm_frame* __restrict__ frames = a.frames;
    const int64_t t_first = tile * (int64_t)(kPlanarThreads * G);
    /* wave-uniform: the frames [f_lo, f_hi) that can hold an element of this workgroup */
    int64_t f_lo = planar_frame_at(frames, 0, a.n_frames, s, t_first);
    if (f_lo < 0) f_lo = 0;
    const int64_t f_hi = planar_frame_at(frames, f_lo, a.n_frames, s, t_first + kPlanarThreads * G - 1) + 1;
    const int64_t len = a.lengths ? a.lengths[s] : INT64_MAX;
    const int64_t t0 = t_first + (int64_t)threadIdx.x * G;
    if (t0 >= a.pitch) return; /* pitch is a multiple of G */
    int64_t f = f_lo - 1; /* f < f_lo: no frame yet */
    flacmi_pcm_frame fr{};
    if (t0 < len && f_lo < f_hi) {
        f = f_hi - f_lo == 1 ? f_lo : planar_frame_at(frames, f_lo, f_hi, s, t0);
        if (f >= f_lo) fr = frames[f];
    }
    const float scale = __int_as_float((127 - (a.sample_size - 1)) << 23); /* 2^-(sample_size - 1) */
    T v[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const int64_t t = t0 + j;
        int32_t x = 0;
        if (t < len && f_lo < f_hi) { /* elements from the stream's length to the pitch stay 0 */
            /* frames of one sample: a group may hold G of them */
            while (f + 1 < f_hi && (f < f_lo || t >= fr.first_sample + fr.block_size || fr.reserved0 != s)) {
                const flacmi_pcm_frame nx = frames[f + 1];
                if (nx.reserved0 > s || (nx.reserved0 == s && nx.first_sample > t)) break;
                fr = nx;
                ++f;
            }
            const int64_t k = t - fr.first_sample;
            if (f >= f_lo && fr.reserved0 == s && k >= 0 && k < fr.block_size && k < fr.stride) {
                x = reinterpret_cast<const int32_t*>(fr.rows)[c * fr.stride + k];
                if (ELEM == FLACMI_PLANAR_INT16 && (x < -32768 || !(x <= 32767))) a.status[f] = FLACMI_STATUS_OVERFLOW;
            }
        }
        if constexpr (ELEM == FLACMI_PLANAR_FLOAT32) v[j] = (float)x * scale;
        else v[j] = (T)x;
    }
    /* every 16-byte group of the row is stored once, whole */
    T* __restrict__ dst = reinterpret_cast<T*>(a.out) + row * a.pitch + t0;
    uint4 q;
    __builtin_memcpy(&q, v, 16);
    *reinterpret_cast<uint4*>(dst) = q;
}

hipError_t launch_planar(PlanarArgs a, int32_t elem, hipStream_t s) {
    if (a.n_frames > 0) {
        hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int32_t) * (size_t)a.n_frames, s);
        if (e != hipSuccess) return e;
    }
    const int sb = elem == FLACMI_PLANAR_INT16 ? 2 : 4;
    const int64_t per = (int64_t)kPlanarThreads * (16 / sb);
    a.tiles = (a.pitch + per - 1) / per;
    const int64_t n = a.tiles * a.n_streams * a.channels;
    if (n <= 0) return hipSuccess;
    const dim3 g((unsigned)n), b(kPlanarThreads);
    if (elem == FLACMI_PLANAR_INT16) hipLaunchKernelGGL((k_planar<int16_t, FLACMI_PLANAR_INT16>), g, b, 0, s, a);
    else if (elem == FLACMI_PLANAR_INT32) hipLaunchKernelGGL((k_planar<int32_t, FLACMI_PLANAR_INT32>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_planar<float, FLACMI_PLANAR_FLOAT32>), g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace flacmi
