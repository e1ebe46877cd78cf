/* decode_bits.h — the frame parsers' shared reader: the decode sites and their status words,
 * the MSB-first bit reader with the fused CRC-16, and the CRC-16 over byte ranges.  Included
 * by k_decode.hip (the decoder) and k_info.hip (the stream report). */
#pragma once
#include "device_common.h"

namespace flacmi {

enum : int32_t {
    DS_SYNC = FLACMI_DSITE_SYNC, DS_BS_CODE, DS_SR_CODE, DS_CH_CODE, DS_SS_CODE, DS_RESERVED,
    DS_SUB_PAD, DS_SUB_TYPE, DS_LPC_PREC, DS_CODING, DS_PARTS, DS_ESC_ZERO, DS_NEG_SHIFT,
    DS_PADDING, DS_EOF, DS_CRC8, DS_CRC16, DS_FRAME_END, DS_FRAME_NO, DS_BLOCK_SIZE, DS_CHANNELS,
    DS_SAMPLES, DS_PCM_RANGE, DS_SIDE_RANGE,
};
static_assert(DS_SAMPLES == FLACMI_DSITE_SAMPLES && DS_SIDE_RANGE == FLACMI_DSITE_SIDE_RANGE, "flacmi_decode_site order");

__device__ __forceinline__ int32_t dstat(int32_t site) {
    int32_t s;
    if (site == DS_EOF) s = FLACMI_STATUS_EOF;
    else if (site == DS_CODING || site == DS_ESC_ZERO || site == DS_NEG_SHIFT) s = FLACMI_STATUS_VALUE_ERROR;
    else if (site >= DS_CRC8) s = FLACMI_STATUS_VERIFY;
    else s = FLACMI_STATUS_ASSERTION;
    return (site << 16) | s;
}
__device__ __forceinline__ bool is_ref_error(int32_t st) { return st != 0 && (st & 0xFFFF) != FLACMI_STATUS_VERIFY; }

/* SAMPLE_SIZE_DECODING (common.py:249-258); code 3 is rejected before */
__device__ __forceinline__ int sample_size_of(int code) {
    switch (code) {
        case 1: return 8;
        case 2: return 12;
        case 4: return 16;
        case 5: return 20;
        case 6: return 24;
        case 7: return 32;
        default: return 0;
    }
}

/* MSB-first reader over the stream: (hi, lo) are dwords b and b + 1 and the read position
 * is 32 b + 32 - sh, sh in [0, 31], so the next 32 bits are one v_alignbit. */
struct BitReader {
    const uint32_t* w;
    int64_t nw;
    int64_t b;
    uint32_t hi, lo;
    int32_t sh;
    int64_t bnear; /* b >= bnear: a 32-bit read could pass the stream's end */
    bool near;
    /* CRC-16 of the frame folded as whole dwords leave the window, in stream order: dword
     * cnext is the next one due, dwords below cend are inside the CRC range (crc16_fused) */
    const uint16_t* ct = nullptr;
    uint32_t crc = 0;
    int64_t cnext = 0, cend = 0;
    __device__ __forceinline__ uint32_t ld(int64_t i) const {
        return (uint64_t)i < (uint64_t)nw ? __builtin_bswap32(w[i]) : 0u;
    }
    __device__ __forceinline__ void fold(uint32_t be) { /* one whole big-endian dword */
        const uint32_t v = be ^ (crc << 16);
        crc = ct[3 * 256 + (v >> 24)] ^ ct[2 * 256 + ((v >> 16) & 0xFF)] ^ ct[256 + ((v >> 8) & 0xFF)] ^ ct[v & 0xFF];
    }
    __device__ __forceinline__ int64_t pos() const { return 32 * b + 32 - sh; }
    __device__ __forceinline__ void seek(int64_t p, int64_t end_bit) {
        b = (p - 1) >> 5; /* p = 0: dword -1 (reads as 0) */
        sh = (int32_t)(32 * b + 32 - p);
        hi = ld(b);
        lo = ld(b + 1);
        bnear = (end_bit >> 5) - 1;
        near = b >= bnear;
    }
    __device__ __forceinline__ void adv() { /* dword b leaves the window */
        if (ct && b == cnext && b < cend) {
            fold(hi);
            ++cnext;
        }
        hi = lo;
        lo = ld(b + 2);
        ++b;
        near = near || b >= bnear;
    }
    /* the 32 bits at the read position, MSB first */
    __device__ __forceinline__ uint32_t peek32() const { return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh); }
    __device__ __forceinline__ void skip(int n) { /* 0 <= n <= 32 */
        sh -= n;
        if (sh < 0) {
            sh += 32;
            adv();
        }
    }
    __device__ __forceinline__ uint32_t uint(int n) { /* 0 <= n <= 32 (binary.py:97) */
        if (n == 0) return 0;
        const uint32_t v = peek32() >> (32 - n);
        skip(n);
        return v;
    }
    __device__ __forceinline__ uint64_t uint64(int n) { /* 0 <= n <= 64 */
        if (n <= 32) return uint(n);
        const uint64_t hi2 = uint(n - 32);
        return (hi2 << 32) | uint(32);
    }
    /* binary.py:129-131 (n >= 1) */
    __device__ __forceinline__ int64_t sint(int n) {
        const uint64_t x = uint64(n);
        return n >= 64 ? (int64_t)x : (int64_t)(x << (64 - n)) >> (64 - n);
    }
    /* get_rice_int (decoder.py:414-421) followed by zigzag_decode (utils.py); sets eof when
     * the unary run passes `end` (the stream's last bit: the reference raises EOFError). */
    __device__ __forceinline__ int64_t rice(int p, int64_t end, bool& eof) {
        uint64_t q = 0;
        uint32_t W = peek32();
        while (W == 0) {
            q += 32;
            skip(32);
            if (pos() > end) {
                eof = true;
                return 0;
            }
            W = peek32();
        }
        const int z = __builtin_clz(W);
        q += z;
        uint64_t v;
        if (z + 1 + p <= 32) {
            v = (q << p) | (p ? ((W << (z + 1)) >> (32 - p)) : 0u);
            skip(z + 1 + p);
        } else {
            skip(z + 1);
            v = (q << p) | uint(p);
        }
        return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
    }
};

/* CRC-16 (crc.py:25-31) of stream bytes [b0, b1), continuing from c: slice-by-4 over
 * whole dwords */
__device__ uint32_t crc16_more(const DecodeArgs& a, const uint16_t* t, uint32_t c, int64_t b0, int64_t b1) {
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(a.words);
    int64_t i = b0;
    for (; i < b1 && (i & 3); ++i) c = ((c << 8) & 0xFFFF) ^ t[((c >> 8) ^ bytes[i]) & 0xFF];
    for (; i + 4 <= b1; i += 4) {
        const uint32_t v = __builtin_bswap32(a.words[i >> 2]) ^ (c << 16);
        c = t[3 * 256 + (v >> 24)] ^ t[2 * 256 + ((v >> 16) & 0xFF)] ^ t[256 + ((v >> 8) & 0xFF)] ^ t[v & 0xFF];
    }
    for (; i < b1; ++i) c = ((c << 8) & 0xFFFF) ^ t[((c >> 8) ^ bytes[i]) & 0xFF];
    return c;
}

/* CRC-16 (crc.py:25-31) of stream bytes [b0, b1): slice-by-4 over whole dwords */
__device__ uint32_t crc16_range(const DecodeArgs& a, const uint16_t* t, int64_t b0, int64_t b1) {
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(a.words);
    uint32_t c = 0;
    int64_t i = b0;
    for (; i < b1 && (i & 3); ++i) c = ((c << 8) & 0xFFFF) ^ t[((c >> 8) ^ bytes[i]) & 0xFF];
    for (; i + 4 <= b1; i += 4) {
        const uint32_t v = __builtin_bswap32(a.words[i >> 2]) ^ (c << 16);
        c = t[3 * 256 + (v >> 24)] ^ t[2 * 256 + ((v >> 16) & 0xFF)] ^ t[256 + ((v >> 8) & 0xFF)] ^ t[v & 0xFF];
    }
    for (; i < b1; ++i) c = ((c << 8) & 0xFFFF) ^ t[((c >> 8) ^ bytes[i]) & 0xFF];
    return c;
}

}  // namespace flacmi
