/* k_rice.hip — the exact Rice search (FLACMI_FLAG_RICE_SEARCH, include/flacmi.h).
 *
 * The reference's find_rice_parameter (encoder.py:730-753) takes floor(log2(sum / len)): it has no
 * value when a partition's zig-zag sum is 0, goes negative when the mean is below 1, may return 31
 * (the 5-bit escape code) and is not the minimum.  The mode replaces it with the parameter that
 * makes the partition smallest, which has no failure site.  For a unit of n samples whose zig-zag
 * residual is row[P .. n), every candidate order o (encoder.py:664-667) and every partition p of it
 * (split_samples_in_partitions) of len_p values z_i:
 *   c_p(k) = sum_i (z_i >> k) + (1 + k) len_p          (= sum rice_size(z_i, k), encoder.py:756-760)
 *   c4_p = min over k in 0..14, c5_p = min over k in 0..30, each at its smallest k
 *   W4(o) = sum_p (4 + c4_p), W5(o) = sum_p (5 + c5_p)
 * and the unit takes the first strictly smallest W walking o upwards, method 4 before method 5.
 *
 *   k_rice_search    one workgroup a unit (the grid loops over the batch), after the analysis
 *                    kernels, which leave the chosen zig-zag row in memory and, where the reference's
 *                    Rice step raises, the choice in the meta record.  sum_i (z_i >> k) =
 *                    sum_{b >= k} 2^(b - k) cnt_b with cnt_b the number of values whose bit b is
 *                    set, so one pass over the row (16-byte loads) counts the bit planes 0..29 of
 *                    every finest partition and sums z >> 30 (k stops at 30); the counts live in
 *                    LDS (132 bytes a finest partition).  Each order's partitions then run
 *                    D(30) = sum (z >> 30), D(k) = cnt_k + 2 D(k + 1) over every k, a workgroup sum gives W4 and W5, and
 *                    the counts of partition pairs are added in place for the next coarser order.
 *                    Nothing is pruned: every k of every partition of every order is evaluated.
 *                    Sums are uint64: a partition's sum of zig-zag values stays below 2^63 (the
 *                    analysis' own bound: sample_bits + qlp_precision <= 44, blocks <= 65535).
 */
#include "device_common.h"

namespace flacmi {

constexpr int kRiceThreads = 256;
constexpr int kRiceParts = 256;  /* finest partitions: rice_max <= 8 with the flag (validate) */
constexpr int kRicePlanes = 30;  /* bit planes counted; the planes above enter as z >> 30 */
static_assert(kRiceThreads >= kRiceParts, "one thread a partition");
static_assert(kRiceThreads % 64 == 0, "whole waves");

/* Add a task's plane counts to partition `part`.  w[2 s + h] holds the counts of the planes
 * s + 8 h (low half) and s + 8 h + 16 (high half), s in 0..7. */
__device__ __forceinline__ void rice_flush(uint32_t* cnt, unsigned long long* hi, int pitch, int part,
                                           const uint32_t (&w)[16], uint64_t h) {
#pragma unroll
    for (int b = 0; b < kRicePlanes; ++b) {
        const uint32_t c = (w[2 * (b & 7) + ((b >> 3) & 1)] >> (16 * (b >> 4))) & 0xffffu;
        if (c) atomicAdd(&cnt[b * pitch + part], c);
    }
    if (h) atomicAdd(&hi[part], (unsigned long long)h);
}

/* T: uint32_t or uint64_t residual rows */
template <typename T>
__global__ __launch_bounds__(kRiceThreads) void k_rice_search(const RiceArgs a) {
    constexpr int G = 16 / (int)sizeof(T); /* values of one 16-byte load */
    constexpr int R = 4 * G;               /* values of one task: 64 bytes of the row */
    union Task {
        uint4 v[4];
        T e[R];
    };
    /* dynamic LDS, sized by the call's finest order (pitch = 2^rice_max partitions: 132 bytes each), so the
     * common ranges leave the CU's LDS to eight workgroups */
    extern __shared__ unsigned long long rice_lds[];
    const int pitch = a.pitch;
    unsigned long long* const hi = rice_lds;                                /* [pitch] sum (z >> 30) per partition */
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(hi + pitch);          /* [plane][pitch] */
    uint8_t* const kp4 = reinterpret_cast<uint8_t*>(cnt + kRicePlanes * pitch); /* [(1 << o) + p]: method 4's parameters */
    uint8_t* const kp5 = kp4 + 2 * pitch;                                   /* and method 5's */
    __shared__ unsigned long long red[3][kRiceThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
        flacmi_unit_meta* const m = a.meta + u;
        const int status = m->status, site = m->site;
        const bool rescue = status == ST_VALUE && (site == FLACMI_SITE_RICE_LOG_DOMAIN || site == FLACMI_SITE_RICE_NEG_SHIFT);
        if (status != ST_OK && !rescue) continue; /* the same in every thread: no barrier is skipped by some */
        const int n = u >= a.n_units - a.n_tail_units ? a.tail_len : a.block_len;
        const int P = status == ST_OK ? m->res_offset : a.mode == FLACMI_MODE_RICE_ONLY ? a.rice_order : m->order;
        int omax = -1; /* both conditions only get harder with o: the candidates are rmin .. omax */
        for (int o = a.rmin; o <= a.rmax; ++o)
            if ((n & ((1 << o) - 1)) == 0 && (n >> o) > P) omax = o;
        if (omax < 0 || P < 0) continue;
        const int F = 1 << omax, plen = n >> omax;

        if (tid < F) {
#pragma unroll
            for (int b = 0; b < kRicePlanes; ++b) cnt[b * pitch + tid] = 0;
            hi[tid] = 0;
        }
        __syncthreads();

        /* ---- the bit-plane counts of the finest partitions: value i belongs to partition i / plen ---- */
        const T* const row = reinterpret_cast<const T*>(a.residual) + u * a.residual_stride;
        if (plen % R == 0) {
            /* a task lies inside one partition.  Four planes a register (bytes), 16 values at most */
            const int ntask = n / R;
            for (int base = wid * 64; base < ntask; base += kRiceThreads) {
                const int t = base + lane, i0 = t * R;
                uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                uint64_t h = 0;
                if (t < ntask) {
                    Task x;
#pragma unroll
                    for (int j = 0; j < 4; ++j) x.v[j] = *reinterpret_cast<const uint4*>(row + i0 + j * G);
#pragma unroll
                    for (int e = 0; e < R; ++e) {
                        const T z = i0 + e >= P ? x.e[e] : (T)0;
                        const uint32_t lo = (uint32_t)z;
#pragma unroll
                        for (int s = 0; s < 8; ++s) c[s] += (lo >> s) & 0x01010101u;
                        h += (uint64_t)(z >> 30);
                    }
                }
                uint32_t w[16];
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    w[2 * s] = c[s] & 0x00ff00ffu;
                    w[2 * s + 1] = (c[s] >> 8) & 0x00ff00ffu;
                }
                const int last = base + 63 < ntask ? base + 63 : ntask - 1;
                const int p0 = base * R / plen, p1 = last * R / plen;
                if (p0 == p1) {
                    /* the wave's 64 tasks share a partition: sum over the lanes (<= 1024 a plane), one lane adds */
#pragma unroll
                    for (int s = 0; s < 16; ++s) w[s] = wave_sum_u32(w[s]);
                    h = wave_sum_u64(h);
                    if (lane == 0) rice_flush(cnt, hi, pitch, p0, w, h);
                } else if (t < ntask) {
                    rice_flush(cnt, hi, pitch, i0 / plen, w, h);
                }
            }
        } else {
            /* any other shape (short or odd blocks): value by value */
            for (int i = P + tid; i < n; i += kRiceThreads) {
                const T z = row[i];
                const int part = i / plen;
                const uint32_t lo = (uint32_t)z;
#pragma unroll
                for (int b = 0; b < kRicePlanes; ++b)
                    if ((lo >> b) & 1u) atomicAdd(&cnt[b * pitch + part], 1u);
                if (z >> 30) atomicAdd(&hi[part], (unsigned long long)(z >> 30));
            }
        }
        __syncthreads();

        /* ---- every order from the finest down: parameters, W4 and W5, then the pairs' counts ---- */
        uint64_t best_w = ~0ull;
        int best_o = omax, best_m = 4;
        for (int o = omax; o >= a.rmin; --o) {
            const int np = 1 << o;
            uint64_t w4 = 0, w5 = 0;
            if (tid < np) {
                const uint64_t len = (uint64_t)((n >> o) - (tid == 0 ? P : 0));
                uint64_t D = hi[tid];
                uint64_t c5 = D + 31 * len, c4 = ~0ull;
                int k5 = 30, k4 = 14;
#pragma unroll
                for (int k = kRicePlanes - 1; k >= 0; --k) {
                    D = 2 * D + cnt[k * pitch + tid];
                    const uint64_t c = D + (uint64_t)(k + 1) * len;
                    if (c <= c5) { /* downwards with <=: the smallest k that reaches the minimum */
                        c5 = c;
                        k5 = k;
                    }
                    if (k <= 14 && c <= c4) {
                        c4 = c;
                        k4 = k;
                    }
                }
                kp4[np + tid] = (uint8_t)k4;
                kp5[np + tid] = (uint8_t)k5;
                w4 = 4 + c4;
                w5 = 5 + c5;
            }
            w4 = wave_sum_u64(w4);
            w5 = wave_sum_u64(w5);
            if (lane == 0) {
                red[0][wid] = w4;
                red[1][wid] = w5;
            }
            /* the pairs' sums, read before the barrier and stored behind it (in place) */
            const int half = np >> 1, items = o > a.rmin ? kRicePlanes * half : 0;
            constexpr int kMerge = kRicePlanes * (kRiceParts / 2) / kRiceThreads;
            uint32_t mc[kMerge];
            uint64_t mh = 0;
#pragma unroll
            for (int j = 0; j < kMerge; ++j) {
                const int i = tid + j * kRiceThreads;
                mc[j] = 0;
                if (i < items) {
                    const int b = i >> (o - 1), p = i & (half - 1);
                    mc[j] = cnt[b * pitch + 2 * p] + cnt[b * pitch + 2 * p + 1];
                }
            }
            if (items && tid < half) mh = hi[2 * tid] + hi[2 * tid + 1];
            __syncthreads();
            w4 = w5 = 0;
#pragma unroll
            for (int k = 0; k < kRiceThreads / 64; ++k) {
                w4 += red[0][k];
                w5 += red[1][k];
            }
            /* walking the orders upwards, method 4 before 5, the first strictly smallest wins: downwards, <= */
            if (w5 <= best_w) {
                best_w = w5;
                best_o = o;
                best_m = 5;
            }
            if (w4 <= best_w) {
                best_w = w4;
                best_o = o;
                best_m = 4;
            }
#pragma unroll
            for (int j = 0; j < kMerge; ++j) {
                const int i = tid + j * kRiceThreads;
                if (i < items) cnt[(i >> (o - 1)) * pitch + (i & (half - 1))] = mc[j];
            }
            if (items && tid < half) hi[tid] = mh;
            __syncthreads();
        }

        /* ---- the result: parameters, the Rice fields of the record, the rescue ---- */
        const int np = 1 << best_o;
        int k = 0;
        if (tid < np) {
            k = (best_m == 5 ? kp5 : kp4)[np + tid];
            a.rice_params[u * a.params_stride + tid] = k;
        }
        const uint64_t over = wave_sum_u64(k > 14 ? 1u : 0u);
        if (lane == 0) red[2][wid] = over;
        __syncthreads();
        if (tid == 0) {
            uint64_t cnt14 = 0;
#pragma unroll
            for (int j = 0; j < kRiceThreads / 64; ++j) cnt14 += red[2][j];
            /* the reference's estimate convention (encoder.py:714-727), so sub_residual_bits returns W */
            m->rice_bits = (int64_t)(best_m == 5 ? best_w + 3ull * np + cnt14 : best_w + 4ull * np);
            m->part_order = best_o;
            m->n_parts = np;
            m->coding_method = best_m;
            m->res_offset = P;
            m->res_len = n - P;
            if (rescue) {
                m->status = ST_OK;
                m->site = FLACMI_SITE_NONE;
            }
        }
        __syncthreads(); /* kp, red and the counts are the next unit's */
    }
}

hipError_t launch_rice_search(const RiceArgs& a, int residual_bytes, int grid_cap, hipStream_t s) {
    if (a.n_units <= 0) return hipSuccess;
    /* memory-bound: 8 workgroups a CU at most, the grid loops over the rest */
    const int64_t cap = grid_cap > 0 ? grid_cap : 2048;
    const dim3 g((unsigned)(a.n_units < cap ? a.n_units : cap)), t(kRiceThreads);
    RiceArgs b = a;
    b.pitch = 1 << (a.rmax < 0 ? 0 : a.rmax > 8 ? 8 : a.rmax);
    const size_t lds = (size_t)b.pitch * (8 + 4 * kRicePlanes + 4);
    if (residual_bytes == 4) hipLaunchKernelGGL(k_rice_search<uint32_t>, g, t, lds, s, b);
    else hipLaunchKernelGGL(k_rice_search<uint64_t>, g, t, lds, s, b);
    return hipGetLastError();
}

}  // namespace flacmi
