/* k_info.hip — the stream report on the device: what each frame of a FLAC stream holds
 * (flac-py README, known issue 3: "a tool providing information about a FLAC file, as
 * `flac -a` does").
 *
 *   k_frame_info  one LANE per frame start, 64 frames per workgroup, grid-stride over the
 *                 list, as k_decode.  The lane walks its frame exactly as the reference's
 *                 get_frame does (decoder.py:111-130, :133-262 the header, :267-355
 *                 subframes, :358-421 the residual) with decode_general's reader and its
 *                 status catalogue, and restores nothing: no history ring, no coefficient
 *                 table, no row stores, no comparison.  What it read goes out instead: one
 *                 flacmi_frame_info per frame, one flacmi_subframe_info per subframe, one
 *                 byte per Rice partition.
 *
 * Only frame starts come in.  The frame ends where the parse stops, so the CRC-16 cannot be
 * fused against a proposed end as decode_general does: whole dwords are folded as they leave
 * the bit window up to the byte-aligned position in front of the footer (every dword folded
 * by then lies wholly before it), the few bytes from there to the footer are folded
 * directly, and the footer is read with the fold switched off.  Both CRCs are reported
 * beside the stored ones and never become a status (the reference reads them unchecked).
 *
 * Status: the exceptions get_frame itself raises, first one wins, plus EOFError.  A negative
 * LPC shift is no error here (the reference raises it in _decode_prediction, after
 * get_frame): the shift is reported as read. */
#include "decode_bits.h"

namespace flacmi {

constexpr int kInfoThreads = 64; /* one wave per workgroup: lanes are independent frames */
constexpr int kInfoGrid = 2048;  /* workgroups at most: longer lists take the grid-stride loop */

/* CRC-16 (crc.py:25-31) of stream bytes [b0, b1), continuing from c (crc16_more of
 * decode_bits.h over a bare word pointer) */
__device__ uint32_t crc16_span(const uint32_t* words, const uint16_t* t, uint32_t c, int64_t b0, int64_t b1) {
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(words);
    int64_t i = b0;
    for (; i < b1 && (i & 3); ++i) c = ((c << 8) & 0xFFFF) ^ t[((c >> 8) ^ bytes[i]) & 0xFF];
    for (; i + 4 <= b1; i += 4) {
        const uint32_t v = __builtin_bswap32(words[i >> 2]) ^ (c << 16);
        c = t[3 * 256 + (v >> 24)] ^ t[2 * 256 + ((v >> 16) & 0xFF)] ^ t[256 + ((v >> 8) & 0xFF)] ^ t[v & 0xFF];
    }
    for (; i < b1; ++i) c = ((c << 8) & 0xFFFF) ^ t[((c >> 8) ^ bytes[i]) & 0xFF];
    return c;
}

/* SAMPLE_RATE_VALUE_DECODING (common.py:149-163) in Hz; code 11 is 96 kHz (flacmi.h) */
__device__ __forceinline__ int32_t sample_rate_of(int code) {
    switch (code) {
        case 1: return 88200;
        case 2: return 176400;
        case 3: return 192000;
        case 4: return 8000;
        case 5: return 16000;
        case 6: return 22050;
        case 7: return 24000;
        case 8: return 32000;
        case 9: return 44100;
        case 10: return 48000;
        case 11: return 96000;
        default: return 0;
    }
}

__device__ void frame_info(const InfoArgs& a, const int64_t f, const uint16_t* crct) {
    const int64_t F = a.offsets[f];
    const int64_t end_bit = a.stream_bytes * 8; /* reading past it: EOFError */
    int64_t coded = 0, fend = -1;
    int32_t bs = 0, strategy = 0, rate = 0, ssize = 0, ch_code = 0, nsub = 0, hdr_bytes = 0;
    int32_t crc8_stored = 0, crc8_computed = 0, crc16_stored = 0, crc16_computed = 0, padding = 0;
    BitReader g;
    g.w = a.words;
    g.nw = a.n_words;
    const int64_t Fh = (F + 3) & ~(int64_t)3;
    /* a parse failure after the reader ran off the stream is the EOFError of that read */
    auto err = [&](int32_t site) { return dstat(g.pos() > end_bit ? (int32_t)DS_EOF : site); };

    auto parse = [&]() -> int32_t {
        if (F < 0 || a.n_words < 1) return dstat(DS_EOF); /* no such byte */
        if (F < a.stream_bytes) { /* the CRC-16's unaligned head now, whole dwords as they leave the window */
            g.ct = crct;
            g.crc = crc16_span(a.words, crct, 0u, F, Fh < a.stream_bytes ? Fh : a.stream_bytes);
            g.cnext = Fh >> 2;
            g.cend = INT64_MAX;
        }
        g.seek(F * 8, end_bit);

        /* ---- frame header (decoder.py:133-245) ---- */
        if (g.uint(15) != 0x7FFC) return err(DS_SYNC);
        strategy = (int32_t)g.uint(1);
        const int bcode = g.uint(4);
        if (!(bcode > 0 && bcode < 15)) return err(DS_BS_CODE);
        const int rcode = g.uint(4);
        if (rcode == 15) return err(DS_SR_CODE);
        ch_code = g.uint(4);
        if (ch_code > 10) return err(DS_CH_CODE);
        const int scode = g.uint(3);
        if (scode == 3) return err(DS_SS_CODE);
        if (g.uint(1) != 0) return err(DS_RESERVED);
        /* coded number (coded_number.py:45-70), as decode_general reads it */
        const uint32_t b0 = g.uint(8);
        const int extra = b0 >= 0xFE ? 6 : b0 >= 0xFC ? 5 : b0 >= 0xF8 ? 4 : b0 >= 0xF0 ? 3 : b0 >= 0xE0 ? 2 : b0 >= 0xC0 ? 1 : 0;
        uint64_t fno = extra == 0 ? b0 : (b0 & ((1u << (6 - extra)) - 1));
        for (int k = 0; k < extra; ++k) fno = (fno << 6) | (g.uint(8) & 0x3F);
        coded = (int64_t)fno;
        if (bcode == 1) bs = 192;
        else if (bcode <= 5) bs = 144 << bcode;
        else if (bcode == 6) bs = (int)g.uint(8) + 1;
        else if (bcode == 7) bs = (int)g.uint(16) + 1;
        else bs = 1 << bcode;
        if (rcode == 12) rate = (int32_t)g.uint(8);
        else if (rcode == 13) rate = (int32_t)g.uint(16);
        else if (rcode == 14) rate = (int32_t)g.uint(16) * 10;
        else rate = sample_rate_of(rcode);
        const int covered = (int)((g.pos() >> 3) - F); /* byte-aligned here: the bytes the CRC-8 covers */
        crc8_stored = (int32_t)g.uint(8);
        if (g.pos() > end_bit) return dstat(DS_EOF);
        hdr_bytes = covered + 1;
        {
            const uint8_t* bytes = reinterpret_cast<const uint8_t*>(a.words);
            uint32_t c = 0; /* x^8 + x^2 + x + 1, init 0 (crc.py:18-22) */
            for (int k = 0; k < covered; ++k) {
                c ^= bytes[F + k];
                for (int b = 0; b < 8; ++b) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
            }
            crc8_computed = (int32_t)c;
        }
        ssize = sample_size_of(scode);
        const int ss = scode == 0 ? a.sample_size : ssize;
        /* an L_R frame holds a.channels subframes (flacmi.h, above FLACMI_STATUS_EOF) */
        const int nch = ch_code == 1 ? a.channels : ch_code <= 7 ? ch_code + 1 : 2;

        /* ---- subframes (decoder.py:267-421) ---- */
        for (int c = 0; c < nch; ++c) {
            const bool keep = c < a.channels; /* a row of a.channels records per frame */
            flacmi_subframe_info* sp = a.subs + (f * a.channels + (keep ? c : 0));
            uint8_t* pp = a.parts ? a.parts + (f * a.channels + (keep ? c : 0)) * (int64_t)a.part_stride : nullptr;
            if (keep) {
                uint64_t* z = reinterpret_cast<uint64_t*>(sp->coefficients); /* 8-byte aligned: offset 40 of 152 */
#pragma unroll
                for (int k = 0; k < 8; ++k) z[k] = 0;
            }
            const int64_t sub0 = g.pos();
            const bool dbit = (ch_code == 8 && c == 1) || (ch_code == 9 && c == 0) || (ch_code == 10 && c == 1);
            if (g.uint(1) != 0) return err(DS_SUB_PAD);
            const int t = g.uint(6);
            if (!(t <= 1 || (t >= 8 && t <= 12) || t >= 32)) return err(DS_SUB_TYPE);
            int wasted = 0;
            if (g.uint(1)) { /* get_wasted_bits: count zeros up to a one */
                while (g.uint(1) == 0) {
                    ++wasted;
                    if (g.pos() > end_bit) break;
                }
                if (a.wasted_spec) ++wasted; /* FLACMI_DECODE_WASTED_SPEC: k is coded as k - 1 zeros and a one */
            }
            const int w = ss + (dbit ? 1 : 0) - wasted; /* sample_size_ (decoder.py:273) */
            /* sint(w <= 0) raises; FIXED order 0 reads no sample at that width (as decode_general) */
            if (w <= 0 && (a.wasted_spec || t != 8)) return err(DS_ESC_ZERO);
            const int order = t >= 32 ? (t & 31) + 1 : t >= 8 ? (t & 7) : 0;
            int64_t cval = 0, rbits = 0;
            uint64_t asum = 0;
            int prec = 0, shift = 0, pbits = 0, po = 0, nesc = 0, stored = 0;
            if (t == 0) {
                cval = g.sint(w);
            } else if (t == 1) {
                int64_t left = (int64_t)bs * w; /* the samples are not looked at */
                while (left > 0) {
                    const int n = left > 32 ? 32 : (int)left;
                    g.skip(n);
                    left -= n;
                    if (g.pos() > end_bit) return dstat(DS_EOF);
                }
            } else {
                for (int k = 0; k < order; ++k) (void)g.sint(w); /* warm-up */
                if (t >= 32) {
                    const int pf = g.uint(4);
                    if (pf == 15) return err(DS_LPC_PREC);
                    prec = pf + 1;
                    shift = (int)g.sint(5);
                    for (int k = 0; k < order; ++k) {
                        const int16_t q = (int16_t)g.sint(prec);
                        if (keep) sp->coefficients[k] = q;
                    }
                }
                const int64_t r0 = g.pos();
                const int cm = g.uint(2);
                if (cm > 1) return err(DS_CODING);
                pbits = cm ? 5 : 4;
                po = g.uint(4);
                if ((bs & ((1 << po) - 1)) != 0 || (bs >> po) <= order) return err(DS_PARTS);
                if (g.pos() > end_bit) return dstat(DS_EOF);
                const int plen = bs >> po, esc_code = (1 << pbits) - 1;
                for (int p = 0; p < (1 << po); ++p) { /* get_rice_partition (decoder.py:397-411) */
                    const int n = p == 0 ? plen - order : plen;
                    const int param = g.uint(pbits);
                    const bool put = keep && pp && p < a.part_stride;
                    stored += put ? 1 : 0;
                    if (param == esc_code) {
                        const int width = g.uint(5);
                        if (width == 0) return err(DS_ESC_ZERO);
                        ++nesc;
                        if (put) pp[p] = (uint8_t)(0x80 | width);
                        for (int i = 0; i < n; ++i) {
                            const int64_t r = g.sint(width);
                            asum += r < 0 ? 0 - (uint64_t)r : (uint64_t)r;
                            if (g.pos() > end_bit) return dstat(DS_EOF);
                        }
                    } else {
                        if (put) pp[p] = (uint8_t)param;
                        for (int i = 0; i < n; ++i) {
                            bool eof = false;
                            const int64_t r = g.rice(param, end_bit, eof);
                            if (eof) return dstat(DS_EOF);
                            asum += r < 0 ? 0 - (uint64_t)r : (uint64_t)r;
                            if (g.pos() > end_bit) return dstat(DS_EOF);
                        }
                    }
                }
                rbits = g.pos() - r0;
            }
            if (g.pos() > end_bit) return dstat(DS_EOF);
            if (keep) {
                sp->bit_offset = sub0 - 8 * F;
                sp->bits = g.pos() - sub0;
                sp->type = t == 0 ? FLACMI_SUB_TYPE_CONSTANT : t == 1 ? FLACMI_SUB_TYPE_VERBATIM : t < 32 ? FLACMI_SUB_TYPE_FIXED : FLACMI_SUB_TYPE_LPC;
                sp->order = order;
                sp->wasted_bits = wasted;
                sp->sample_bits = w;
                sp->precision = prec;
                sp->shift = shift;
                sp->coding_method = pbits;
                sp->partition_order = po;
                sp->escaped_partitions = nesc;
                sp->reserved0 = 0;
                sp->residual_bits = rbits;
                sp->abs_sum = (int64_t)asum;
                sp->constant_value = cval;
                sp->partitions_stored = stored;
                sp->reserved1 = 0;
            }
            ++nsub;
        }

        /* ---- footer (decoder.py:124-128): zero padding to a byte, CRC-16 ---- */
        if (g.pos() & 7) {
            padding = 8 - (int)(g.pos() & 7);
            if (g.uint(padding) != 0) return err(DS_PADDING);
        }
        if (g.pos() > end_bit) return dstat(DS_EOF);
        {
            const int64_t E = g.pos() >> 3; /* the CRC-16 covers [F, E) */
            const int64_t lo = 4 * g.cnext; /* dwords [Fh / 4, cnext) are folded: all below E */
            const uint32_t c = (E <= Fh || lo > E) ? crc16_span(a.words, crct, 0u, F, E) : crc16_span(a.words, crct, g.crc, lo, E);
            crc16_computed = (int32_t)c;
            g.ct = nullptr; /* the footer is outside the range */
        }
        crc16_stored = (int32_t)g.uint(16);
        if (g.pos() > end_bit) return dstat(DS_EOF);
        fend = g.pos() >> 3;
        return 0;
    };
    const int32_t st = parse();

    flacmi_frame_info* o = a.frames + f;
    o->offset = F;
    o->end = st ? -1 : fend;
    o->coded_number = coded;
    o->status = st;
    o->block_size = bs;
    o->blocking_strategy = strategy;
    o->sample_rate = rate;
    o->sample_size = ssize;
    o->channel_code = ch_code;
    o->n_subframes = nsub;
    o->header_bytes = hdr_bytes;
    o->crc8_stored = crc8_stored;
    o->crc8_computed = crc8_computed;
    o->crc16_stored = st ? 0 : crc16_stored;
    o->crc16_computed = st ? 0 : crc16_computed;
    o->padding_bits = padding;
    o->reserved0 = 0;
}

__global__ __launch_bounds__(kInfoThreads) void k_frame_info(InfoArgs a) {
    __shared__ uint16_t crct[4 * 256];
    const int lane = threadIdx.x;
    for (int i = lane; i < 4 * 256; i += kInfoThreads) crct[i] = a.crc_slice[i];
    __syncthreads();
    for (int64_t k = (int64_t)blockIdx.x * kInfoThreads + lane; k < a.n_frames; k += (int64_t)gridDim.x * kInfoThreads)
        frame_info(a, k, crct);
}

hipError_t launch_frame_info(const InfoArgs& a, int grid_cap, hipStream_t s) {
    if (a.n_frames <= 0) return hipSuccess;
    int64_t blocks = (a.n_frames + kInfoThreads - 1) / kInfoThreads;
    const int64_t cap = grid_cap > 0 ? grid_cap : kInfoGrid;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_frame_info, dim3((unsigned)blocks), dim3(kInfoThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace flacmi
