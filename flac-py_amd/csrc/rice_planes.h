/* rice_planes.h — the bit-plane steps of the exact Rice search (FLACMI_FLAG_RICE_SEARCH,
 * include/flacmi.h), shared by k_rice_search (k_rice.hip: the chosen row of an analysed unit) and
 * k_size_choice (k_size.hip: every candidate's residual of a unit).
 *
 * For zig-zag values z_i of a partition, sum_i (z_i >> k) = sum_{b >= k} 2^(b - k) cnt_b with cnt_b
 * the number of values whose bit b is set: the bit planes 0..29 of every finest partition are
 * counted once and the planes above enter as sum (z >> 30) (k stops at 30).  The counts live in LDS
 * (132 bytes a finest partition).  Each order's partitions then run D(30) = sum (z >> 30),
 * D(k) = cnt_k + 2 D(k + 1) over every k, a workgroup sum gives W4 and W5, and the counts of
 * partition pairs are added in place for the next coarser order.  Nothing is pruned.  Sums are
 * uint64: a partition's sum of zig-zag values stays below 2^63 (the analysis' own bound:
 * sample_bits + qlp_precision <= 44, blocks <= 65535).
 */
#pragma once
#include "device_common.h"

namespace flacmi {

constexpr int kRiceThreads = 256;
constexpr int kRiceParts = 256;  /* finest partitions: rice_max <= 8 with the flag (validate) */
constexpr int kRicePlanes = 30;  /* bit planes counted; the planes above enter as z >> 30 */
static_assert(kRiceThreads >= kRiceParts, "one thread a partition");
static_assert(kRiceThreads % 64 == 0, "whole waves");

/* The search's LDS tables for `pitch` = 2^rice_max finest partitions, carved from 8-byte aligned
 * dynamic LDS: rice_lds_bytes(pitch) bytes. */
struct RiceLds {
    unsigned long long* hi; /* [pitch] sum (z >> 30) per partition */
    uint32_t* cnt;          /* [plane][pitch] */
    uint8_t* kp4;           /* [(1 << o) + p]: method 4's parameters */
    uint8_t* kp5;           /* and method 5's */
};
__host__ __device__ constexpr size_t rice_lds_bytes(int pitch) { return (size_t)pitch * (8 + 4 * kRicePlanes + 4); }
__device__ __forceinline__ RiceLds rice_lds_carve(unsigned long long* base, int pitch) {
    RiceLds l;
    l.hi = base;
    l.cnt = reinterpret_cast<uint32_t*>(l.hi + pitch);
    l.kp4 = reinterpret_cast<uint8_t*>(l.cnt + kRicePlanes * pitch);
    l.kp5 = l.kp4 + 2 * pitch;
    return l;
}

/* Largest candidate partition order of a unit of n samples at predictor order P (encoder.py:664-667;
 * both conditions only get harder with o: the candidates are rmin .. the result), -1 with none */
__device__ __forceinline__ int rice_omax(int n, int P, int rmin, int rmax) {
    int omax = -1;
    for (int o = rmin; o <= rmax; ++o)
        if ((n & ((1 << o) - 1)) == 0 && (n >> o) > P) omax = o;
    return omax;
}

/* Zero the counts of the F finest partitions (the caller's barrier follows) */
__device__ __forceinline__ void rice_zero(const RiceLds& l, int pitch, int F, int tid) {
    if (tid < F) {
#pragma unroll
        for (int b = 0; b < kRicePlanes; ++b) l.cnt[b * pitch + tid] = 0;
        l.hi[tid] = 0;
    }
}

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

/* One value into partition `part`, plane by plane (short or odd shapes) */
__device__ __forceinline__ void rice_count_value(uint32_t* cnt, unsigned long long* hi, int pitch, int part, uint64_t z) {
    const uint32_t lo = (uint32_t)z;
#pragma unroll
    for (int b = 0; b < kRicePlanes; ++b)
        if ((lo >> b) & 1u) atomicAdd(&cnt[b * pitch + part], 1u);
    if (z >> 30) atomicAdd(&hi[part], (unsigned long long)(z >> 30));
}

/* The 64 values of a wave that all lie in partition `part`: one ballot a plane, lane b adds plane b */
__device__ __forceinline__ void rice_count_wave(uint32_t* cnt, unsigned long long* hi, int pitch, int part, uint64_t z,
                                                int lane) {
    const uint32_t lo = (uint32_t)z;
    uint32_t mine = 0;
#pragma unroll
    for (int b = 0; b < kRicePlanes; ++b) {
        const uint32_t c = (uint32_t)__popcll(__ballot((lo >> b) & 1u));
        mine = lane == b ? c : mine;
    }
    const uint64_t h = wave_sum_u64(z >> 30);
    if (lane < kRicePlanes && mine) atomicAdd(&cnt[lane * pitch + part], mine);
    if (lane == kRicePlanes && h) atomicAdd(&hi[part], (unsigned long long)h);
}

/* Every order from omax (whose 1 << omax partitions' counts are in l, behind a barrier) down to
 * rmin: each partition's parameters into kp4 / kp5, W4 and W5, then the pairs' counts.  Walking the
 * orders upwards, method 4 before 5, the first strictly smallest W wins (downwards: <=).  Called by
 * the whole workgroup; every thread gets the same result; ends behind a barrier.  The counts are
 * consumed. */
__device__ __forceinline__ void rice_walk(const RiceLds& l, unsigned long long (*red)[kRiceThreads / 64], int pitch, int n,
                                          int P, int rmin, int omax, int tid, uint64_t& best_w, int& best_o,
                                          int& best_m) {
    const int lane = tid & 63, wid = tid >> 6;
    uint32_t* const cnt = l.cnt;
    unsigned long long* const hi = l.hi;
    best_w = ~0ull;
    best_o = omax;
    best_m = 4;
    for (int o = omax; o >= rmin; --o) {
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
            l.kp4[np + tid] = (uint8_t)k4;
            l.kp5[np + tid] = (uint8_t)k5;
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
        const int half = np >> 1, items = o > rmin ? kRicePlanes * half : 0;
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
}

/* meta.rice_bits of a searched unit: the reference's estimate convention (encoder.py:714-727), so
 * sub_residual_bits returns W.  over = #{k_p > 14} */
__device__ __forceinline__ int64_t rice_estimate_bits(uint64_t W, int method, int np, uint64_t over) {
    return (int64_t)(method == 5 ? W + 3ull * np + over : W + 4ull * np);
}

}  // namespace flacmi
