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
 *                    Rice step raises, the choice in the meta record.  One pass over the row (16-byte
 *                    loads) counts the bit planes 0..29 of every finest partition and sums z >> 30;
 *                    the plane counts, each order's minimum over k and the merge of partition pairs
 *                    are rice_planes.h (shared with k_size_choice).  Nothing is pruned: every k of
 *                    every partition of every order is evaluated.
 */
#include "rice_planes.h"

namespace flacmi {

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
    const RiceLds l = rice_lds_carve(rice_lds, pitch);
    unsigned long long* const hi = l.hi;
    uint32_t* const cnt = l.cnt;
    __shared__ unsigned long long red[3][kRiceThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
        flacmi_unit_meta* const m = a.meta + u;
        const int status = m->status, site = m->site;
        const bool rescue = status == ST_VALUE && (site == FLACMI_SITE_RICE_LOG_DOMAIN || site == FLACMI_SITE_RICE_NEG_SHIFT);
        if (status != ST_OK && !rescue) continue; /* the same in every thread: no barrier is skipped by some */
        const int n = u >= a.n_units - a.n_tail_units ? a.tail_len : a.block_len;
        const int P = status == ST_OK ? m->res_offset : a.mode == FLACMI_MODE_RICE_ONLY ? a.rice_order : m->order;
        const int omax = rice_omax(n, P, a.rmin, a.rmax);
        if (omax < 0 || P < 0) continue;
        const int F = 1 << omax, plen = n >> omax;

        rice_zero(l, pitch, F, tid);
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
                rice_count_value(cnt, hi, pitch, i / plen, (uint64_t)row[i]);
            }
        }
        __syncthreads();

        /* ---- every order from the finest down: parameters, W4 and W5, then the pairs' counts ---- */
        uint64_t best_w;
        int best_o, best_m;
        rice_walk(l, red, pitch, n, P, a.rmin, omax, tid, best_w, best_o, best_m);

        /* ---- the result: parameters, the Rice fields of the record, the rescue ---- */
        const int np = 1 << best_o;
        int k = 0;
        if (tid < np) {
            k = (best_m == 5 ? l.kp5 : l.kp4)[np + tid];
            a.rice_params[u * a.params_stride + tid] = k;
        }
        const uint64_t over = wave_sum_u64(k > 14 ? 1u : 0u);
        if (lane == 0) red[2][wid] = over;
        __syncthreads();
        if (tid == 0) {
            uint64_t cnt14 = 0;
#pragma unroll
            for (int j = 0; j < kRiceThreads / 64; ++j) cnt14 += red[2][j];
            m->rice_bits = rice_estimate_bits(best_w, best_m, np, cnt14);
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
    const size_t lds = rice_lds_bytes(b.pitch);
    if (residual_bytes == 4) hipLaunchKernelGGL(k_rice_search<uint32_t>, g, t, lds, s, b);
    else hipLaunchKernelGGL(k_rice_search<uint64_t>, g, t, lds, s, b);
    return hipGetLastError();
}

}  // namespace flacmi
