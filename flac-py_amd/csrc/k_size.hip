/* k_size.hip — the subframe choice by exact written size (FLACMI_FLAG_SIZE_CHOICE, include/flacmi.h).
 *
 * The reference picks the fixed order (encoder.py:350-352), the LPC order (:398-404) and the
 * subframe type (:135-157) by sum |r|; its TODO in encode() (:104-118) wants the size of the
 * subframe instead.  The mode takes, among the fixed orders 0..4 and (FLACMI_MODE_REFERENCE) the
 * LPC orders 1..L of k_lpc's record, the first candidate with the strictly smallest
 *   bits = 8 + P ss + (LPC: 9 + P q) + 6 + W
 * with W the exact Rice search's written size of that candidate's zig-zag residual
 * (rice_planes.h: the same walk and parameter ties as k_rice_search).
 *
 *   k_size_choice    one workgroup a unit (the grid loops over the batch), behind k_lpc; neither
 *                    k_resid nor k_rice_search runs in such a call.  The unit's samples and its
 *                    LPC record are copied to LDS once.  Per eligible candidate: the taps go to
 *                    LDS, every thread forms residuals from the LDS samples (64-bit sums), their
 *                    zig-zag values are counted into the bit planes of the finest partitions (a wave
 *                    whose 64 values share a partition: one ballot a plane and one add a plane;
 *                    otherwise value by value), and rice_walk gives W; no zig-zag value is stored.
 *                    The first strictly smallest candidate keeps its order, method and parameters
 *                    (256 bytes of LDS).  The winner's residual is then formed once more and
 *                    written as the row (16-byte stores), with the parameters and the whole record.
 *                    Correctness first: nothing is pruned, nothing is tuned.
 */
#include "rice_planes.h"

namespace flacmi {

/* byte offsets (multiples of 16) behind the Rice tables in the dynamic LDS */
struct SizeLds {
    int bestk, cf, rec, xs, total;
};
__host__ __device__ inline SizeLds size_lds_layout(int block_len, int sample_bytes, int rec_words, int pitch) {
    auto up = [](int b) { return (b + 15) & ~15; };
    SizeLds l;
    int o = up((int)rice_lds_bytes(pitch));
    l.bestk = o; o = up(o + pitch);                          /* the best candidate's parameters */
    l.cf = o;    o = up(o + 4 * (FLACMI_MAX_LPC_ORDER + 1)); /* the candidate's taps, then its shift */
    l.rec = o;   o = up(o + 4 * rec_words);                  /* the unit's LPC record */
    l.xs = o;    o = up(o + block_len * sample_bytes);       /* its samples */
    l.total = o;
    return l;
}

/* candidate taps: fixed order P (c_fixed_coef, shift 0) or the record's LPC order P */
__device__ __forceinline__ void size_taps(int32_t* cf, const int32_t* recl, int L, bool lpc, int P, int tid) {
    if (tid < FLACMI_MAX_LPC_ORDER)
        cf[tid] = lpc ? (tid < P ? recl[2 + L + (P * (P - 1)) / 2 + tid] : 0) : (tid < 4 ? c_fixed_coef[P][tid] : 0);
    if (tid == FLACMI_MAX_LPC_ORDER) cf[tid] = lpc ? recl[2 + P - 1] : 0;
}

/* prediction_residual (encoder.py:537-548) at i >= P */
template <typename S>
__device__ __forceinline__ int64_t size_resid(const S* xs, const int32_t* cf, int P, int shift, int i) {
    int64_t pred = 0;
    for (int j = 0; j < P; ++j) pred += (int64_t)cf[j] * (int64_t)xs[i - 1 - j];
    return (int64_t)xs[i] - (pred >> shift);
}

/* the whole record, field by field (no local struct: keeps the kernel scratch-free) */
__device__ __forceinline__ void size_put_meta(flacmi_unit_meta* m, int status, int site, int kind, int order, int shift,
                                              int ncoefs, const int32_t* cf, int res_offset, int res_len, int ford,
                                              int lord, int part_order, int n_parts, int coding, int64_t fsum,
                                              int64_t lsum, int64_t rice_bits) {
    m->status = status;
    m->site = site;
    m->kind = kind;
    m->order = order;
    m->shift = shift;
    m->ncoefs = ncoefs;
    m->res_offset = res_offset;
    m->res_len = res_len;
    m->fixed_order = ford;
    m->lpc_order = lord;
    m->part_order = part_order;
    m->n_parts = n_parts;
    m->coding_method = coding;
    m->lpc_tiers = 0;
    m->fixed_sum = fsum;
    m->lpc_sum = lsum;
    m->rice_bits = rice_bits;
    for (int j = 0; j < FLACMI_MAX_LPC_ORDER; ++j) m->coefs[j] = j < ncoefs ? cf[j] : 0;
}

/* S: int16_t or int32_t samples; T: uint32_t or uint64_t residual rows */
template <typename S, typename T>
__global__ __launch_bounds__(kRiceThreads) void k_size_choice(const SizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long size_lds[];
    __shared__ unsigned long long red[3][kRiceThreads / 64];
    const int pitch = a.pitch;
    const RiceLds l = rice_lds_carve(size_lds, pitch);
    const SizeLds lay = size_lds_layout(a.block_len, (int)sizeof(S), a.rec_words, pitch);
    char* const lds = reinterpret_cast<char*>(size_lds);
    uint8_t* const bestk = reinterpret_cast<uint8_t*>(lds + lay.bestk);
    int32_t* const cf = reinterpret_cast<int32_t*>(lds + lay.cf);
    int32_t* const recl = reinterpret_cast<int32_t*>(lds + lay.rec);
    S* const xs = reinterpret_cast<S*>(lds + lay.xs);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const bool ref = a.mode == FLACMI_MODE_REFERENCE;
    const int L = ref ? a.L : 0;
    constexpr int G = 16 / (int)sizeof(T); /* values of one 16-byte store */

    for (int64_t u = blockIdx.x; u < a.n_units; u += gridDim.x) {
        const int n = u >= a.n_units - a.n_tail_units ? a.tail_len : a.block_len;
        flacmi_unit_meta* const m = a.meta + u;
        /* rows are 16-byte aligned at a pitch of whole 16 bytes: the last load stays inside the row's pitch */
        const uint4* const src = reinterpret_cast<const uint4*>(reinterpret_cast<const S*>(a.samples) + u * a.stride);
        const int nv = (n * (int)sizeof(S) + 15) / 16;
        for (int v = tid; v < nv; v += kRiceThreads) reinterpret_cast<uint4*>(xs)[v] = src[v];
        if (ref)
            for (int i = tid; i < a.rec_words; i += kRiceThreads) recl[i] = a.rec[u * a.rec_words + i];
        __syncthreads();
        const int st_rec = ref ? recl[0] : 0;
        if (st_rec != 0) { /* the reference raises inside encode_subframe_lpc, before any choice */
            if (tid == 0) put_meta(m, st_rec & 0xffff, st_rec >> 16, nullptr, 0);
            __syncthreads(); /* the record and the samples are the next unit's */
            continue;
        }
        const uint32_t negmask = ref ? (uint32_t)recl[1] : 0u;
        if (a.lpc_sums && tid >= L && tid < FLACMI_MAX_LPC_ORDER) a.lpc_sums[u * 32 + tid] = 0;

        /* ---- every candidate in order: fixed 0..4, LPC 1..L ---- */
        int64_t best_bits = -1, fbits = -1, lbits = -1;
        uint64_t best_w = 0;
        int best_c = -1, best_o = 0, best_m = 4, ford = -1, lord = -1;
        for (int c = 0; c < 5 + L; ++c) {
            const bool lpc = c >= 5;
            const int P = lpc ? c - 4 : c;
            /* not a candidate: a fixed order above 0 of a unit of at most 4 samples (encoder.py:334); an LPC
             * order of the quantiser's negative-shift branch (written undecodably); any at q = 16 (:619) */
            const bool cand = lpc ? (((negmask >> (P - 1)) & 1u) == 0 && a.q != 16) : (c == 0 || n > 4);
            const int omax = cand ? rice_omax(n, P, a.rmin, a.rmax) : -1;
            int64_t bits = -1;
            if (omax >= 0) {
                size_taps(cf, recl, L, lpc, P, tid);
                rice_zero(l, pitch, 1 << omax, tid);
                __syncthreads();
                const int shift = cf[FLACMI_MAX_LPC_ORDER], plen = n >> omax;
                for (int b0 = P + wid * 64; b0 < n; b0 += kRiceThreads) { /* b0: the same in a wave */
                    const int i = b0 + lane;
                    uint64_t z = 0;
                    if (i < n) {
                        const int64_t r = size_resid(xs, cf, P, shift, i);
                        z = ((uint64_t)r << 1) ^ (uint64_t)(r >> 63);
                    }
                    const int last = b0 + 63 < n ? b0 + 63 : n - 1;
                    const int p0 = b0 / plen;
                    if (p0 == last / plen) rice_count_wave(l.cnt, l.hi, pitch, p0, z, lane);
                    else if (i < n) rice_count_value(l.cnt, l.hi, pitch, i / plen, z);
                }
                __syncthreads();
                uint64_t w;
                int o, mth;
                rice_walk(l, red, pitch, n, P, a.rmin, omax, tid, w, o, mth);
                bits = 8 + (int64_t)P * a.ss + (lpc ? 9 + (int64_t)P * a.q : 0) + 6 + (int64_t)w;
                if (best_c < 0 || bits < best_bits) { /* the first strictly smallest */
                    best_bits = bits;
                    best_c = c;
                    best_w = w;
                    best_o = o;
                    best_m = mth;
                    if (tid < (1 << o)) bestk[tid] = (mth == 5 ? l.kp5 : l.kp4)[(1 << o) + tid];
                }
                if (lpc && (lord < 0 || bits < lbits)) {
                    lbits = bits;
                    lord = P;
                }
                if (!lpc && (ford < 0 || bits < fbits)) {
                    fbits = bits;
                    ford = P;
                }
            }
            if (tid == 0) {
                if (!lpc && a.fixed_sums) a.fixed_sums[u * 5 + c] = bits;
                if (lpc && a.lpc_sums) a.lpc_sums[u * 32 + P - 1] = bits;
            }
        }
        if (!ref) {
            lord = 0;
            lbits = 0;
        }
        if (best_c < 0) { /* no candidate has a partition order */
            if (tid == 0)
                size_put_meta(m, ST_ASSERT, FLACMI_SITE_RICE_NO_ORDER, 0, 0, 0, 0, cf, 0, 0, ford, lord, 0, 0, 0, fbits,
                              lbits, 0);
            __syncthreads();
            continue;
        }

        /* ---- the winner: its residual once more, as the row; parameters; record ---- */
        const bool lpc = best_c >= 5;
        const int P = lpc ? best_c - 4 : best_c;
        size_taps(cf, recl, L, lpc, P, tid);
        __syncthreads();
        const int shift = cf[FLACMI_MAX_LPC_ORDER];
        T* const rout = reinterpret_cast<T*>(a.residual) + u * a.residual_stride;
        int wide = 0;
        for (int i0 = tid * G; i0 < n; i0 += kRiceThreads * G) {
            T zv[G];
#pragma unroll
            for (int e = 0; e < G; ++e) {
                const int i = i0 + e;
                T z = 0;
                if (i >= P && i < n) {
                    const int64_t r = size_resid(xs, cf, P, shift, i);
                    if constexpr (sizeof(T) == 4) {
                        if (!(r >= -(1LL << 31) && r < (1LL << 31))) wide = 1;
                        const int32_t r32 = (int32_t)r;
                        z = (T)(((uint32_t)r32 << 1) ^ (uint32_t)(r32 >> 31));
                    } else {
                        z = (T)(((uint64_t)r << 1) ^ (uint64_t)(r >> 63));
                    }
                }
                zv[e] = z;
            }
            if (i0 + G <= n) {
                uint4 q;
                if constexpr (sizeof(T) == 4) {
                    q = uint4{(uint32_t)zv[0], (uint32_t)zv[1], (uint32_t)zv[2], (uint32_t)zv[3]};
                } else {
                    q = uint4{(uint32_t)zv[0], (uint32_t)((uint64_t)zv[0] >> 32), (uint32_t)zv[1],
                              (uint32_t)((uint64_t)zv[1] >> 32)};
                }
                *reinterpret_cast<uint4*>(rout + i0) = q;
            } else {
#pragma unroll
                for (int e = 0; e < G; ++e)
                    if (i0 + e < n) rout[i0 + e] = zv[e];
            }
        }
        wide = __syncthreads_or(wide);
        const int np = 1 << best_o;
        const int k = tid < np ? bestk[tid] : 0;
        const int over = __syncthreads_count(k > 14);
        const int kind = lpc ? FLACMI_KIND_LPC : FLACMI_KIND_FIXED, ncoefs = lpc ? P : 0;
        if (sizeof(T) == 4 && wide) { /* the caller's redo on 8-byte rows carries the flag */
            if (tid == 0)
                size_put_meta(m, FLACMI_STATUS_RESIDUAL_WIDE, FLACMI_SITE_RESIDUAL_WIDTH, kind, P, shift, ncoefs, cf, 0, 0,
                              ford, lord, 0, 0, 0, fbits, lbits, 0);
        } else {
            if (tid < np) a.rice_params[u * a.params_stride + tid] = k;
            if (tid == 0)
                size_put_meta(m, ST_OK, FLACMI_SITE_NONE, kind, P, shift, ncoefs, cf, P, n - P, ford, lord, best_o, np,
                              best_m, fbits, lbits, rice_estimate_bits(best_w, best_m, np, (uint64_t)over));
        }
        __syncthreads(); /* every LDS table is the next unit's */
    }
}

size_t size_choice_lds(int block_len, int sample_bytes, int rec_words, int rmax) {
    return (size_t)size_lds_layout(block_len, sample_bytes, rec_words, 1 << (rmax < 0 ? 0 : rmax > 8 ? 8 : rmax)).total;
}

hipError_t launch_size_choice(const SizeArgs& a, int residual_bytes, int grid_cap, hipStream_t s) {
    if (a.n_units <= 0) return hipSuccess;
    const int64_t cap = grid_cap > 0 ? grid_cap : 2048;
    const dim3 g((unsigned)(a.n_units < cap ? a.n_units : cap)), t(kRiceThreads);
    SizeArgs b = a;
    b.pitch = 1 << (a.rmax < 0 ? 0 : a.rmax > 8 ? 8 : a.rmax);
    const size_t lds = size_choice_lds(a.block_len, a.sample_bytes, a.rec_words, a.rmax);
    auto kern = a.sample_bytes == 2 ? (residual_bytes == 4 ? k_size_choice<int16_t, uint32_t> : k_size_choice<int16_t, uint64_t>)
                                    : (residual_bytes == 4 ? k_size_choice<int32_t, uint32_t> : k_size_choice<int32_t, uint64_t>);
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, g, t, lds, s, b);
    return hipGetLastError();
}

}  // namespace flacmi
