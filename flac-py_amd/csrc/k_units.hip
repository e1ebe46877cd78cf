/* k_units.hip — the decoder's rows as the encoder's unit rows (flacmi_units_out_device).
 *
 * The counterpart of k_pcm (k_index.hip): the same frame list (planar int32 rows, each frame
 * with its own pitch, first_sample and block_size), re-cut into blocks of another length
 * without leaving the device.  Sample s >= S0 of channel c goes to unit ((s - S0) / B) * C + c,
 * element (s - S0) % B.
 *
 * One workgroup per output unit (a gather), not one per frame (a scatter, as k_pcm does):
 *   - a workgroup writes its own row and nothing else, so whatever the frame list holds no
 *     byte outside the n_units rows is written, and the zero fill from the unit's length to
 *     the pitch is the same loop as the samples (every 16-byte group of the row is stored
 *     exactly once, whole);
 *   - a frame boundary may fall anywhere inside a 16-byte group; a scatter would have to
 *     write such a group from two workgroups in parts.
 * The unit passes through LDS in tiles of kUnitsTile elements, already narrowed to the row type:
 * the gather reads one element per lane (a wave reads 64 consecutive int32 of a source row,
 * coalesced whatever the source offset; a lane that gathers its own 16-byte group reads 8
 * dwords 32 bytes apart from its neighbour's), the store reads 16 bytes per lane from LDS and
 * writes 16 bytes.
 * The price of the gather is finding the frames: the frames that can hold the unit's first and
 * last sample are found by two wave-uniform binary searches over first_sample (scalar loads,
 * the same for every lane).  A unit inside one frame keeps that frame's record in scalar
 * registers; otherwise a lane searches only that range for its sample (one step for a unit over
 * two frames, nine when it holds 300 one-sample frames).  No scratch.
 *
 * Range check: a sample read that does not fit sample_size bits sets its frame's status word
 * (every finder writes the same value).  Measured width: the maximum over the samples written
 * of x >= 0 ? x : ~x, reduced per wave, then an atomic max into one word by the waves that
 * would raise it. */
#include "flacmi_kernels.h"

namespace flacmi {

/* the largest f in [lo, hi) whose first_sample <= s, or lo - 1 */
__device__ __forceinline__ int64_t units_frame_at(const flacmi_pcm_frame* __restrict__ fr, int64_t lo, int64_t hi,
                                                  int64_t s) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (fr[mid].first_sample <= s) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

constexpr int kUnitsTile = 4096; /* elements of a unit row staged in LDS at a time */

template <typename T>
__global__ __launch_bounds__(256) void k_units(UnitsArgs a) {
    constexpr int G = 16 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) T tile[kUnitsTile];
    const int64_t u = blockIdx.x;
    const int64_t blk = u / a.channels;
    const int c = (int)(u - blk * a.channels);
    const int len = blk < a.n_blocks ? a.block_len : a.tail_len;
    const int64_t s_begin = a.s0 + blk * (int64_t)a.block_len;
    T* __restrict__ row = reinterpret_cast<T*>(a.units) + u * a.stride;
    const flacmi_pcm_frame* __restrict__ frames = a.frames;
    /* wave-uniform: the frames [f_lo, f_hi) that can hold a sample of this unit */
    int64_t f_lo = units_frame_at(frames, 0, a.n_frames, s_begin);
    if (f_lo < 0) f_lo = 0;
    const int64_t f_hi = units_frame_at(frames, f_lo, a.n_frames, s_begin + (len > 0 ? len - 1 : 0)) + 1;
    const bool one = f_hi - f_lo == 1; /* the whole unit lies in one frame: its record stays in scalar registers */
    flacmi_pcm_frame only{};
    if (one) only = frames[f_lo];
    const int64_t lo = -((int64_t)1 << (a.sample_size - 1)), hi = ((int64_t)1 << (a.sample_size - 1)) - 1;
    uint32_t widest = 0;
    for (int64_t base = 0; base < a.stride; base += kUnitsTile) {
        const int cnt = (int)(a.stride - base < kUnitsTile ? a.stride - base : kUnitsTile); /* a multiple of G */
        /* gather: lane j reads element base + j, so a wave reads 64 consecutive int32 of a source row
         * until a frame ends, wherever the frame starts */
        for (int j = threadIdx.x; j < cnt; j += 256) {
            const int64_t i = base + j;
            int32_t v = 0;
            if (i < len) { /* elements from the unit's length to the pitch stay 0 */
                const int64_t s = s_begin + i;
                int64_t f = f_lo;
                flacmi_pcm_frame fr = only;
                if (!one) {
                    f = units_frame_at(frames, f_lo, f_hi, s);
                    if (f >= f_lo) fr = frames[f];
                }
                const int64_t t = s - fr.first_sample;
                if (t >= 0 && t < fr.block_size && t < fr.stride) {
                    v = reinterpret_cast<const int32_t*>(fr.rows)[c * fr.stride + t];
                    if (v < lo || !(v <= hi)) a.status[f] = FLACMI_STATUS_OVERFLOW;
                    const uint32_t m = (uint32_t)(v >= 0 ? v : ~v);
                    widest = m > widest ? m : widest;
                }
            }
            tile[j] = (T)v;
        }
        __syncthreads();
        /* every 16-byte group of the row is stored once, whole */
        for (int j = threadIdx.x * G; j < cnt; j += 256 * G)
            *reinterpret_cast<uint4*>(row + base + j) = *reinterpret_cast<const uint4*>(tile + j);
        __syncthreads();
    }
    for (int k = 32; k >= 1; k >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)widest, k);
        widest = other > widest ? other : widest;
    }
    /* one word for the whole grid: an atomic per wave serialises at L2 (4e5 of them cost 4 ms of a
     * 4.6 ms launch on 1e5 units), so a wave first reads the word, which only ever grows, and adds
     * its own atomic only where it would raise it: a handful per launch */
    if ((threadIdx.x & 63) == 0 && widest > __atomic_load_n(a.width, __ATOMIC_RELAXED)) atomicMax(a.width, widest);
}

hipError_t launch_units(const UnitsArgs& a, int32_t sample_bytes, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.width, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (a.n_frames > 0) {
        e = hipMemsetAsync(a.status, 0, sizeof(int32_t) * (size_t)a.n_frames, s);
        if (e != hipSuccess) return e;
    }
    const int64_t n_units = (a.n_blocks + (a.tail_len > 0 ? 1 : 0)) * a.channels;
    if (n_units <= 0) return hipSuccess;
    const dim3 g((unsigned)n_units), b(256);
    if (sample_bytes == 2) hipLaunchKernelGGL(k_units<int16_t>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_units<int32_t>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace flacmi
