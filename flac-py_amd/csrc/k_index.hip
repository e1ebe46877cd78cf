/* k_index.hip — the stream decoder's two ends: where frames may start in a byte stream
 * whose offsets nobody kept (k_index_*), and the decoder's planar int32 rows as the
 * interleaved little-endian PCM a WAV file holds (k_pcm).
 *
 * The reference finds frames by reading them: get_frames (decoder.py:100-108) calls
 * get_frame until EOFError, each frame starting where the last one ended, so nothing in a
 * frame can be decoded before every frame ahead of it has been.  A frame header, however,
 * announces itself: a 15-bit sync code, four code fields with reserved values, a coded
 * number and a CRC-8 over all of it (decoder.py:133-185, crc.py:18-22).  k_index lists every
 * byte position whose bytes pass all of that, the "candidates", in stream order; the host
 * then walks from candidate to candidate with the decoded frames' own ends
 * (flacmi_host_chain_walk) and drops the false ones.
 *
 *   k_index_count  a tile is kIndexTile bytes, 16 per lane in one load, four tiles a workgroup
 *              (their loads issued together); the 17th byte the two-byte sync test needs comes
 *              from the next lane (the wave's last lane loads it).  FF bytes followed by F8 / F9
 *              are found with three zero-byte masks per dword, no per-byte loop; the rare
 *              positions that match are parsed on a divergent path (parse_header).  Writes
 *              each tile's count.
 *   k_index_offsets / k_index_groups  exclusive scan of the tile counts in two levels (1024
 *              tiles a workgroup, then the groups' sums in one workgroup), the total count.
 *   k_index_write  the tiles that hold candidates (a uniform early exit for the rest) again,
 *              each candidate written at its tile's base + its rank inside the tile, so the
 *              table is in stream order whatever order the workgroups ran in.
 *
 * k_pcm: one workgroup per frame, one output dword per lane and step, so the stores are
 * whole aligned dwords whatever the sample width, the channel count or the frame's first
 * byte; only the (at most two) dwords a frame shares with its neighbours are written as
 * bytes. */
#include "flacmi_kernels.h"

namespace flacmi {

constexpr int kIdxThreads = kIndexTile / 16;
static_assert(kIdxThreads == 256, "one 16-byte load per lane");
constexpr int kIdxTilesPerGroup = 4; /* count pass: tiles per workgroup (loads in flight per lane) */
constexpr int kIdxScan = 1024;       /* tiles per group of the two-level scan */
int64_t index_scan_groups(int64_t n_tiles) { return (n_tiles + kIdxScan - 1) / kIdxScan; }

/* 0x80 in every byte of v that is zero */
__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) {
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

/* the lane's 16 bytes of the tile (virtual positions count from the 16-byte boundary at or
 * below the base; bytes outside the stream read as 0, which starts no sync code) */
__device__ __forceinline__ void load16(const IndexArgs& a, int64_t v0, uint32_t (&w)[4]) {
    const uint8_t* vb = a.base - a.mis;
    const int64_t lo = a.mis, hi = a.mis + a.bytes;
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (v0 >= lo && v0 + 16 <= hi) {
        const uint4 q = *reinterpret_cast<const uint4*>(vb + v0);
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else if (v0 + 16 > lo && v0 < hi) { /* the stream's first and last 16 bytes */
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t v = v0 + k;
            const uint32_t b = (v >= lo && v < hi) ? vb[v] : 0u;
            w[k >> 2] |= b << (8 * (k & 3));
        }
    }
}

/* 0x80 in byte i of hit[j] where a sync code (FF, then F8 or F9) starts at byte 4 j + i */
__device__ __forceinline__ uint32_t sync_hits(const IndexArgs& a, int64_t v0, int lane, const uint32_t (&w)[4],
                                              uint32_t (&hit)[4]) {
    uint32_t nxt = __shfl_down(w[0], 1);
    if ((lane & 63) == 63) {
        const int64_t v = v0 + 16;
        nxt = (v >= a.mis && v < a.mis + a.bytes) ? (a.base - a.mis)[v] : 0u;
    }
    uint32_t f8[5];
#pragma unroll
    for (int j = 0; j < 4; ++j) f8[j] = zero_bytes((w[j] | 0x01010101u) ^ 0xF9F9F9F9u);
    f8[4] = zero_bytes((((nxt & 0xFFu) | 0x01u) ^ 0xF9u) | 0x01010100u); /* byte 0 only */
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hit[j] = zero_bytes(~w[j]) & ((f8[j] >> 8) | (f8[j + 1] << 24));
        any |= hit[j];
    }
    return any;
}

/* the rare positions with a sync code: parse; f(candidate) for each that passes */
template <typename F>
__device__ __forceinline__ void for_candidates(const IndexArgs& a, int64_t v0, const uint32_t (&hit)[4], F f) {
    flacmi_frame_candidate c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t h = hit[j];
        while (h) {
            const int i = __builtin_ctz(h) >> 3;
            h &= h - 1;
            const int64_t p = v0 + 4 * j + i - a.mis;
            if (p >= a.first && parse_header(a.base, a.bytes, p, true, c)) f(c);
        }
    }
}

/* Count pass: kIdxTilesPerGroup tiles per workgroup, their loads issued together. */
__global__ __launch_bounds__(kIdxThreads) void k_index_count(IndexArgs a) {
    __shared__ int32_t total[kIdxTilesPerGroup];
    const int lane = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * kIdxTilesPerGroup;
    uint32_t w[kIdxTilesPerGroup][4];
#pragma unroll
    for (int k = 0; k < kIdxTilesPerGroup; ++k) load16(a, (tile0 + k) * kIndexTile + 16 * (int64_t)lane, w[k]);
    if (lane < kIdxTilesPerGroup) total[lane] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kIdxTilesPerGroup; ++k) {
        const int64_t v0 = (tile0 + k) * kIndexTile + 16 * (int64_t)lane;
        uint32_t hit[4];
        if (sync_hits(a, v0, lane, w[k], hit)) { /* candidates are rare: the few lanes that hold one add up in LDS */
            int32_t n = 0;
            for_candidates(a, v0, hit, [&](const flacmi_frame_candidate&) { ++n; });
            if (n) atomicAdd(&total[k], n);
        }
    }
    __syncthreads();
    if (lane < kIdxTilesPerGroup && tile0 + lane < a.n_tiles) a.tile_count[tile0 + lane] = total[lane];
}

/* Write pass: the tiles that hold candidates (a uniform early exit for the rest), each
 * candidate at its tile's base + its rank inside the tile. */
__global__ __launch_bounds__(kIdxThreads) void k_index_write(IndexArgs a) {
    __shared__ int32_t wsum[kIdxThreads / 64];
    const int64_t tile = blockIdx.x;
    if (a.tile_count[tile] == 0) return;
    const int lane = threadIdx.x;
    const int64_t v0 = tile * kIndexTile + 16 * (int64_t)lane;
    uint32_t w[4], hit[4];
    load16(a, v0, w);
    int32_t n = 0;
    if (sync_hits(a, v0, lane, w, hit)) for_candidates(a, v0, hit, [&](const flacmi_frame_candidate&) { ++n; });
    /* rank: inclusive scan inside the wave by shuffles, the waves' sums through LDS */
    int32_t incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t u = __shfl_up(incl, d);
        if ((lane & 63) >= d) incl += u;
    }
    if ((lane & 63) == 63) wsum[lane >> 6] = incl;
    __syncthreads();
    if (n == 0) return;
    int64_t slot = a.group_base[tile / kIdxScan] + a.tile_base[tile] + incl - n;
    for (int k = 0; k < (lane >> 6); ++k) slot += wsum[k];
    for_candidates(a, v0, hit, [&](const flacmi_frame_candidate& c) {
        if (slot < a.capacity) a.table[slot] = c;
        ++slot;
    });
}

/* tile_base = exclusive prefix sums of tile_count inside each group of kIdxScan tiles, and the
 * group's sum */
__global__ __launch_bounds__(kIdxScan) void k_index_offsets(IndexArgs a) {
    __shared__ int32_t part[kIdxScan];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * kIdxScan + lane;
    const int32_t n = t < a.n_tiles ? a.tile_count[t] : 0;
    part[lane] = n;
    __syncthreads();
    for (int d = 1; d < kIdxScan; d <<= 1) {
        const int32_t v = lane >= d ? part[lane - d] : 0;
        __syncthreads();
        part[lane] += v;
        __syncthreads();
    }
    if (t < a.n_tiles) a.tile_base[t] = part[lane] - n;
    if (lane == kIdxScan - 1) a.group_base[blockIdx.x] = part[lane];
}

/* group_base: the groups' sums -> their exclusive prefix sums; *count = the total.  One
 * workgroup, kIdxScan groups a step. */
__global__ __launch_bounds__(kIdxScan) void k_index_groups(IndexArgs a) {
    __shared__ int64_t part[kIdxScan];
    __shared__ int64_t carry;
    const int lane = threadIdx.x;
    const int64_t ng = (a.n_tiles + kIdxScan - 1) / kIdxScan;
    if (lane == 0) carry = 0;
    __syncthreads();
    for (int64_t g0 = 0; g0 < ng; g0 += kIdxScan) {
        const int64_t g = g0 + lane;
        const int64_t n = g < ng ? a.group_base[g] : 0;
        part[lane] = n;
        __syncthreads();
        for (int d = 1; d < kIdxScan; d <<= 1) {
            const int64_t v = lane >= d ? part[lane - d] : 0;
            __syncthreads();
            part[lane] += v;
            __syncthreads();
        }
        if (g < ng) a.group_base[g] = carry + part[lane] - n;
        __syncthreads();
        if (lane == kIdxScan - 1) carry += part[lane];
        __syncthreads();
    }
    if (lane == 0) *a.count = carry;
}

hipError_t launch_index(const IndexArgs& a, hipStream_t s) {
    if (a.n_tiles <= 0) return hipMemsetAsync(a.count, 0, sizeof(int64_t), s);
    const unsigned groups = (unsigned)((a.n_tiles + kIdxTilesPerGroup - 1) / kIdxTilesPerGroup);
    hipLaunchKernelGGL(k_index_count, dim3(groups), dim3(kIdxThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_index_offsets, dim3((unsigned)index_scan_groups(a.n_tiles)), dim3(kIdxScan), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_index_groups, dim3(1), dim3(kIdxScan), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_index_write, dim3((unsigned)a.n_tiles), dim3(kIdxThreads), 0, s, a);
    return hipGetLastError();
}

/* ---- k_pcm --------------------------------------------------------------------------- */
/* Frame f's bytes are out[first_sample * channels * B ..) for block_size * channels * B
 * bytes; element e of the frame (e = t * channels + c) is rows[c * stride + t].  A lane
 * owns the aligned output dword d and gathers its 4 bytes from the (at most 4) elements
 * that cover them; the element whose first byte lies in the dword is range-checked there. */
template <int B, bool RAW>
__global__ __launch_bounds__(256) void k_pcm(PcmArgs a) {
    const int64_t f = blockIdx.x;
    const flacmi_pcm_frame fr = a.frames[f];
    const int ch = a.channels;
    const int64_t b0 = fr.first_sample * ch * B, nbytes = (int64_t)fr.block_size * ch * B;
    if (b0 < 0 || b0 + nbytes > a.capacity) { /* never write outside the caller's buffer */
        if (threadIdx.x == 0) a.status[f] = (FLACMI_SITE_FRAME_SIZE << 16) | FLACMI_STATUS_FRAME_TOO_LARGE;
        return;
    }
    const int32_t* rows = reinterpret_cast<const int32_t*>(fr.rows);
    const int64_t d0 = b0 >> 2, d1 = (b0 + nbytes + 3) >> 2; /* dwords [d0, d1) touch the frame */
    bool over = false;
    for (int64_t d = d0 + threadIdx.x; d < d1; d += 256) {
        const int64_t r0 = 4 * d - b0; /* frame-relative byte of the dword's byte 0, may be < 0 */
        int64_t rb = r0 < 0 ? 0 : r0;
        int64_t e = rb / B;
        int k = (int)(rb - e * B);
        int64_t t = e / ch;
        int c = (int)(e - t * ch);
        uint32_t word = 0;
        int32_t v = rb < nbytes ? rows[c * fr.stride + t] : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + j;
            if (r < rb || r >= nbytes) continue;
            if (!RAW && B < 4 && k == 0) over |= v < -((int64_t)1 << (8 * B - 1)) || v >= ((int64_t)1 << (8 * B - 1));
            word |= (((uint32_t)v >> (8 * k)) & 0xFFu) << (8 * j);
            if (++k == B) { /* the next element */
                k = 0;
                if (++c == ch) c = 0, ++t;
                if (r + 1 < nbytes) v = rows[c * fr.stride + t];
            }
        }
        if (r0 >= 0 && r0 + 4 <= nbytes) {
            reinterpret_cast<uint32_t*>(a.out)[d] = word;
        } else { /* a dword shared with the neighbouring frame: this frame's bytes only */
            for (int j = 0; j < 4; ++j)
                if (r0 + j >= 0 && r0 + j < nbytes) a.out[4 * d + j] = (uint8_t)(word >> (8 * j));
        }
    }
    if (over) a.status[f] = FLACMI_STATUS_OVERFLOW; /* every lane writes the same word */
}

hipError_t launch_pcm(const PcmArgs& a, hipStream_t s) {
    if (a.n_frames <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int32_t) * (size_t)a.n_frames, s);
    if (e != hipSuccess) return e;
    const dim3 g((unsigned)a.n_frames), b(256);
    if (a.raw) hipLaunchKernelGGL((k_pcm<4, true>), g, b, 0, s, a);
    else if (a.bytes_per_sample == 1) hipLaunchKernelGGL((k_pcm<1, false>), g, b, 0, s, a);
    else if (a.bytes_per_sample == 2) hipLaunchKernelGGL((k_pcm<2, false>), g, b, 0, s, a);
    else if (a.bytes_per_sample == 3) hipLaunchKernelGGL((k_pcm<3, false>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_pcm<4, false>), g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace flacmi
