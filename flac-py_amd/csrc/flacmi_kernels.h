/*
 * flacmi_kernels.h — internal interface between the host driver (flacmi_host.cpp) and
 * the HIP kernels (flacmi_kernels.hip).  Not part of the public C-ABI.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/flacmi.h"

namespace flacmi {

/* Zero entries behind the n weights of a unit's Tukey window (get_window).  The k_lpc kernels
 * read the window for every slot of their last load block / ring cycle / tile, whose samples
 * at and past n - 1 are loaded as 0: up to one whole block (k_lpc: SB, k_lpc_tile: 64) past
 * n - 1.  At least the largest SB of any build (80: 16-bit samples at LMAX 32); each kernel
 * asserts its own block against it. */
constexpr int kWindowPad = 80;

/* One launch = one "length class": units [unit0, unit0 + count) that all have length n. */
struct LpcArgs {
    const void* samples;     /* batch base pointer */
    int64_t stride;          /* elements between units */
    int64_t unit0, count;
    int32_t sample_bytes;
    int32_t n, L, q;
    const double* window;    /* [n] Tukey(0.5) window for this n (host libm cos) */
    const double* log2thr;   /* [PYM_LOG2_THR_N] floor(log2) thresholds */
    int32_t* rec;            /* [count][rec_words] LPC records (workspace) */
    int32_t rec_words;
    int32_t lpc_sign;        /* FLACMI_FLAG_LPC_SIGN: quantise the negated Levinson coefficients */
    double* acf;             /* optional [count][33] */
    int32_t fuse_lo, fuse_hi; /* window[i] == 1.0 exactly for i in [fuse_lo, fuse_hi) and
                                 |x| < 2^26 (0, 0: no fused blocks), see k_lpc */
    uint32_t* bound;         /* optional [count][kBoundWords]: the energy bound's words for k_resid_stream
                                (lpc_finish); the window then holds kBoundLags more values behind its pad: kappa_1 .. */
};
/* a unit's row of bound words (32 bytes): 0, 1 the energy bound's pair over every order (or the
 * unusable pair below); 2, 3 the same pair over orders 2 .. L alone ((0, 0): L = 1, no such order,
 * which passes); 4 order 1's coefficient and shift, (uint16)c_1 | shift_1 << 16; 5 .. 7 zero.
 * Words 2 .. 4 mean nothing where words 0, 1 are unusable. */
constexpr int kBoundWords = 8;
/* the energy bound: the word pair of a unit it must not decide, and the lags
 * k = 1 .. kBoundLags of kappa_k = max_i |w_i - w_{i-k}| stored at window[n + kWindowPad ..] */
constexpr uint32_t kBoundUnusable = 0xffffffffu;
/* second word of an unusable pair: some order's sum|taps| exceeds kCoefLimit (below), so the
 * stream kernel will list the unit and need not run its fixed group first */
constexpr uint32_t kBoundOutside = 0xfffffffeu;
constexpr int kBoundLags = 13;
/* k_resid_stream's MFMA exactness bound per LPC order: (sum|c| + 2^shift) * 33023 < 2^22.  A
 * unit outside it is listed by the stream kernel; k_lpc gives it unusable bound words */
constexpr int kCoefLimit = 127;

struct ResidArgs {
    const void* samples;
    int64_t stride;
    int64_t unit0, count;
    int32_t sample_bytes;
    int32_t n, L, mode;
    int32_t rmin, rmax;      /* rice range; rmax < rmin => empty */
    int32_t rice_order;      /* predictor order in FLACMI_MODE_RICE_ONLY */
    const int32_t* rec;      /* [count][rec_words] (NULL in fixed-only mode) */
    int32_t rec_words;
    const double* log2thr;
    flacmi_unit_meta* meta;  /* [count] */
    int32_t* rice_params;    /* [count][params_stride] */
    int64_t params_stride;
    void* residual;          /* [count][residual_stride] u32 or u64 */
    int64_t residual_stride;
    int64_t* fixed_sums;     /* optional [count][5] */
    int64_t* lpc_sums;       /* optional [count][32] */
    int32_t stop_after;      /* profiling ablation (env FLACMI_DEBUG_STOP): 0 = full kernel,
                                1 = after staging, 2 = after candidate sums, 3 = after the
                                choice, 4 = after the chosen residual (k_resid config-3
                                Rice phase: 5 = after the parameters, 6 = after the row
                                transform, 7 = after the data bits); k_resid_stream prune
                                mode: 11 = bound tier 0 only, 12 = no LPC bound (wrong
                                results, timing only) */
    int32_t mfma;            /* 1 = MFMA candidate sums where exact (env FLACMI_NO_MFMA=1 -> 0) */
    unsigned long long* retry_count; /* fast-path units handed to the generic kernel: count, */
    int64_t* retry_list;             /* and their batch indices (NULL: no fast path) */
    unsigned long long* retry2_count; /* k_resid_stream: the units its list kernel hands on to k_resid's */
    int64_t* retry2_list;             /* list variant (a second list of at most count entries) */
    unsigned long long* retry_sub;    /* k_resid_stream's batch kernel lists unit u in sub-list u & 63: its
                                         counter retry_sub[16 (u & 63)] (128 B apart), its entries
                                         retry_list[(u & 63) retry_sub_cap ..] (one counter for every
                                         workgroup serialised ~13 ns per listed unit at L2) */
    int64_t retry_sub_cap;
    int32_t sample_bits;             /* declared sample width (bounds the 64-bit paths' narrow sums) */
    int32_t stream;                  /* 1 = k_resid_stream where the shape allows (env FLACMI_NO_STREAM=1 -> 0) */
    int32_t prune;                   /* 1 = reference mode may skip the exact LPC candidate sums of a unit
                                        whose lower bounds already lose to the best fixed sum
                                        (meta lpc_order = lpc_sum = FLACMI_LPC_PRUNED) */
    int32_t persist;                 /* k_resid kVarMf8: the grid loops over the batch and copies the next
                                        unit's samples into LDS (LDS-DMA) during this unit's Rice phase */
    int32_t sign_bound;              /* int8-MFMA pruning: try the sign-correlation bound before the tiers */
    const uint32_t* bound;           /* k_resid_stream's batch kernel: k_lpc's bound words [count][kBoundWords] and */
    const uint16_t* chunk_weight;    /* [n / 8] floor(256 min window weight) per 8-sample chunk (NULL: no pre-test) */
    int32_t energy;                  /* knob FLACMI_ENERGY_BOUND: 1 = both pre-tests (the energy bound over every
                                        order, then orders 2 .. L by it and order 1 by the closed form), then the
                                        tiers; 2 = the first pre-test, then the exact pass; 3 = both, then the exact
                                        pass; 4 = the first, then the tiers; 0 = the tiers alone.  Bit 0: the second
                                        pre-test runs; bit 1: an undecided unit skips the tiers */
    int64_t list_off;                /* k_resid_stream's pre-test build lists unit gid as gid + list_off (set by
                                        the launchers: launch_stream_class_batch) */
};
/* internal unit status between the fast and the generic k_resid (never returned) */
#define FLACMI_STATUS_RETRY 0x7e

/* The stereo mode's verdict on one frame (k_stereo_choose, FLACMI_STEREO_BEST) */
struct StereoChoice {
    int32_t code;            /* channel assignment: 1 L_R, 8 L_S, 9 S_R, 10 M_S (header byte 3 >> 4) */
    int32_t status;          /* non-zero: the frame fails with it (FLACMI_STATUS_RESIDUAL_WIDE on a candidate) */
    int64_t unit[2];         /* the two subframes' candidate units (frame_bits.h: [0, 4 n_frames)) */
};

/* Frame writer (k_frame.hip): frame f = units [f*channels, (f+1)*channels). */
struct FrameArgs {
    const void* samples;     /* warm-up samples come from the batch rows */
    int64_t stride;
    int32_t sample_bytes;
    int32_t block_len, tail_len;
    int64_t n_units, n_tail_units;
    int32_t channels, sample_size, q;
    int64_t first_frame, n_frames;
    const flacmi_unit_meta* meta;
    const int32_t* rice_params;
    int64_t params_stride;
    const void* residual;
    int32_t residual_bytes;
    int64_t residual_stride;
    int64_t* offsets;        /* [n_frames + 1] */
    int32_t* status;         /* [n_frames] */
    uint8_t* out;
    int64_t capacity;
    const uint16_t* crc_slice; /* [4][256] CRC-16 slice-by-4 tables */
    const uint16_t* crc_pow;   /* [28][512] multiply-by-x^(8*2^b) tables */
    int32_t pack_split;        /* 1: k_pack32 writes the frames it can hold, k_pack the rest */
    unsigned long long* slow_count; /* pack_split: frames k_pack32 hands to k_pack: count, */
    int64_t* slow_list;              /* and their indices ([n_frames]) */
    int32_t ablate;            /* profiling only (env FLACMI_PACK_ABLATE): 1 no CRC shift, 2 no residual codes,
                                  3 neither (output invalid) */
    int32_t* sub_kind;         /* FLACMI_FRAME_FALLBACK: [n_units] flacmi_sub_kind, written by k_sub_kinds and
                                  read by k_frame_sizes and the writers; NULL: the mode is off */
    /* FLACMI_STEREO_BEST (choice NULL: the mode is off).  meta, rice_params, the residual rows and
       sub_kind then hold 4 n_frames candidate units: the caller's 2 n_frames, then the mid units,
       then the side units (frame_bits.h); n_units stays the caller's count */
    StereoChoice* choice;      /* [n_frames], written by k_stereo_choose, read by k_frame_sizes_st / k_pack_st */
    const void* mid;           /* mid rows [n_frames], elements of sample_bytes */
    int64_t mid_stride;
    const int32_t* side;       /* side rows [n_frames], sample_size + 1 bits in int32 */
    int64_t side_stride;
    const int32_t* wasted;     /* FLACMI_FRAME_WASTED: [n_units] wasted bits of the units, whose rows are already
                                  shifted right by them (k_wasted_rows); NULL: the mode is off.  Not with choice */
};

/* Decoder verifier (k_decode.hip): frame f = bytes [offsets[f], offsets[f+1]) of words. */
struct DecodeArgs {
    const uint32_t* words;   /* the stream as dwords (4-byte aligned base) */
    int64_t stream_bytes, n_words;
    const int64_t* offsets;  /* [n_frames + 1] */
    int64_t n_frames;
    int32_t channels, sample_size;
    int64_t first_frame;
    int32_t check_crc;
    const void* expect;      /* optional source rows [n_frames*channels][expect_stride] */
    int64_t expect_stride;
    int32_t expect_bytes;
    int32_t expect_vec;      /* rows 16-byte aligned: the comparison uses 16-byte loads */
    int32_t block_len, tail_len;
    int64_t n_units, n_tail_units;
    int32_t* out;            /* optional [n_frames*channels][out_stride] */
    int64_t out_stride;
    int32_t* status;         /* [n_frames] */
    int64_t* mismatch;       /* [n_frames] */
    int32_t* decorr;         /* [n_frames] scratch: (bs << 8) | channel code for k_decorr, else 0 */
    const uint16_t* crc_slice; /* [4][256] CRC-16 slice-by-4 tables */
    unsigned long long* defer_count; /* frames k_decode_fx hands to k_decode: count, */
    int64_t* defer_list;             /* and their indices ([n_frames]) */
    int32_t defer_all;               /* knob FLACMI_DECODE_GENERIC: every frame through k_decode */
    unsigned long long* defer2_count; /* the frames k_decode_fx's LPC pass hands on: count, */
    int64_t* defer2_list;             /* and their indices ([n_frames]) */
    int32_t lpc_pass;                 /* k_decode_fx's LPC pass runs (knob FLACMI_DECODE_LPC=0: off) */
    int64_t* frame_end;               /* optional [n_frames]: the byte after the frame's footer where the
                                         frame raised no reference exception, else -1 */
    int32_t wasted_spec;             /* FLACMI_DECODE_WASTED_SPEC: wasted bits = zeros + 1, shifted back in */
    const int64_t* frame_limit;      /* optional [n_frames] (the batch decoder): the byte where frame f's own stream
                                        ends inside the buffer; k_decode<END, true> raises EOFError there */
};

/* Frame index (k_index.hip): candidate frame starts of a byte stream, in stream order.  A tile
 * is the bytes one workgroup reads (16 per lane); tiles count from the 16-byte boundary at or
 * below the stream's base address. */
constexpr int kIndexTile = 4096;
struct IndexArgs {
    const uint8_t* base;     /* 4-byte aligned */
    int64_t bytes, first;    /* stream size; candidates at offsets >= first only */
    int32_t mis;             /* base address & 15 */
    int64_t n_tiles;         /* ceil((mis + bytes) / kIndexTile) */
    flacmi_frame_candidate* table;
    int64_t capacity;
    int64_t* count;          /* the true count, whatever the capacity */
    int32_t* tile_count;     /* workspace [n_tiles rounded up to 4] */
    int32_t* tile_base;      /* workspace [n_tiles]: exclusive prefix inside the tile's scan group */
    int64_t* group_base;     /* workspace [index_scan_groups(n_tiles)] */
};

/* Every header check of decode_general (k_decode.hip, decoder.py:133-185) at byte p, whose
 * first two bytes are known to hold the sync code, plus (check_crc8) the CRC-8; reads bytes
 * [p, bytes) only.  The device lists candidates with it (k_index.hip); the host reads the
 * block size of a chain frame that is no candidate with it (flacmi_decode_stream_host). */
__host__ __device__ inline bool parse_header(const uint8_t* s, int64_t bytes, int64_t p, bool check_crc8,
                                             flacmi_frame_candidate& c) {
    if (p + 6 > bytes) return false; /* sync, two code bytes, one number byte, CRC-8 */
    const uint32_t b2 = s[p + 2], b3 = s[p + 3];
    const int bcode = b2 >> 4, rcode = b2 & 15, ch = b3 >> 4, scode = (b3 >> 1) & 7;
    if (bcode == 0 || bcode == 15 || rcode == 15 || ch > 10 || scode == 3 || (b3 & 1)) return false;
    const uint32_t b0 = s[p + 4];
    const int extra = b0 >= 0xFE ? 6 : b0 >= 0xFC ? 5 : b0 >= 0xF8 ? 4 : b0 >= 0xF0 ? 3 : b0 >= 0xE0 ? 2 : b0 >= 0xC0 ? 1 : 0;
    const int nb = bcode == 6 ? 1 : bcode == 7 ? 2 : 0, nr = rcode == 12 ? 1 : rcode >= 13 ? 2 : 0;
    const int n = 5 + extra + nb + nr; /* bytes the CRC-8 covers */
    if (p + n + 1 > bytes) return false;
    uint64_t fno = extra == 0 ? b0 : (b0 & ((1u << (6 - extra)) - 1));
    for (int k = 0; k < extra; ++k) fno = (fno << 6) | (s[p + 5 + k] & 0x3F);
    int bs;
    if (bcode == 1) bs = 192;
    else if (bcode <= 5) bs = 144 << bcode;
    else if (bcode == 6) bs = (int)s[p + 5 + extra] + 1;
    else if (bcode == 7) bs = (((int)s[p + 5 + extra] << 8) | s[p + 6 + extra]) + 1;
    else bs = 1 << bcode;
    uint32_t crc = 0; /* x^8 + x^2 + x + 1, init 0 */
    for (int k = 0; k < n; ++k) {
        crc ^= s[p + k];
        for (int b = 0; b < 8; ++b) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1) & 0xFF;
    }
    if (check_crc8 && crc != s[p + n]) return false;
    c.offset = p;
    c.coded_number = (int64_t)fno;
    c.block_size = bs;
    c.header_bytes = n + 1;
    c.channel_code = ch;
    c.sample_size_code = scode;
    return true;
}

/* Stream report (k_info.hip, k_frame_info): one lane per frame start, the parse of
 * decode_general with nothing restored and every field it read written out. */
struct InfoArgs {
    const uint32_t* words;   /* stream bytes (4-byte aligned) */
    int64_t stream_bytes, n_words;
    const int64_t* offsets;  /* [n_frames] frame starts */
    int64_t n_frames;
    int32_t channels, sample_size;
    flacmi_frame_info* frames;   /* [n_frames] */
    flacmi_subframe_info* subs;  /* [n_frames][channels] */
    uint8_t* parts;              /* [n_frames][channels][part_stride], or nullptr */
    int32_t part_stride;
    const uint16_t* crc_slice;   /* [4][256] CRC-16 slice-by-4 tables */
    int32_t wasted_spec;         /* FLACMI_DECODE_WASTED_SPEC: wasted_bits = zeros + 1, sample_bits accordingly */
};

/* PCM writer (k_index.hip, k_pcm) */
struct PcmArgs {
    const flacmi_pcm_frame* frames;
    int64_t n_frames;
    int32_t channels, bytes_per_sample, raw;
    uint8_t* out;            /* 4-byte aligned */
    int64_t capacity;
    int32_t* status;         /* [n_frames] */
};

/* Unit rows from decoded frames (k_units.hip): sample s >= s0 of channel c of the frame list
 * goes to unit ((s - s0) / block_len) * channels + c, element (s - s0) % block_len; n_blocks
 * whole blocks, then one block of tail_len samples when tail_len > 0 */
struct UnitsArgs {
    const flacmi_pcm_frame* frames; /* ordered by first_sample, no gaps */
    int64_t n_frames;
    int32_t channels, block_len, tail_len, sample_size;
    int64_t s0, n_blocks;
    void* units;             /* int16 or int32 rows, 16-byte aligned */
    int64_t stride;          /* elements; a multiple of 16 bytes, >= block_len */
    int32_t* status;         /* [n_frames] */
    uint32_t* width;         /* one word: max over the samples written of x >= 0 ? x : ~x */
};

/* Planar rows from decoded frames (k_planar.hip): sample t of channel c of stream s goes to
 * out[(s * channels + c) * pitch + t]; the frames are ordered by (stream, first_sample), the
 * stream index in flacmi_pcm_frame.reserved0 */
struct PlanarArgs {
    const flacmi_pcm_frame* frames;
    int64_t n_frames, n_streams;
    int32_t channels, sample_size;
    const int64_t* lengths;  /* optional [n_streams]: samples from lengths[s] on are written as 0 */
    void* out;               /* int16, int32 or float rows, 16-byte aligned */
    int64_t pitch;           /* elements; a multiple of 16 bytes */
    int64_t tiles;           /* workgroups per row */
    int32_t* status;         /* [n_frames] */
};

struct ResidLaunch {
    int threads;            /* workgroup size (multiple of 64) */
    size_t lds_bytes;        /* dynamic LDS */
};

/* Launch configuration the residual kernel needs for (n, L, rice range, residual width). */
ResidLaunch resid_launch_config(int n, int rmax_eff, int residual_bytes);
/* Largest partition order the LDS tables support. */
constexpr int kMaxFinestParts = 4096;

/* flacmi_set_knob's knobs: the environment's value (read once) or the last value set */
enum Knob { kKnobOverlap = 0, kKnobMf8Grid, kKnobStreamGeneric, kKnobDecodeGeneric, kKnobPackGeneric, kKnobDecodeLpc, kKnobEnergyBound, kKnobInfoGrid, kKnobRiceGrid, kKnobCount };
int knob(Knob k);

hipError_t launch_lpc(const LpcArgs& a, hipStream_t s);
/* units one full round of launch_lpc's kernel covers on the current device (resident
 * workgroups per CU x 256 units x CUs); 0 when the occupancy query fails */
int64_t lpc_units_per_round(const LpcArgs& a);
/* test knob: fill every CU's LDS with a pattern (env FLACMI_POISON_LDS), else nothing */
hipError_t launch_poison_lds(hipStream_t s);
/* copy nf + 1 frame offsets and nf statuses to mapped host memory (k_misc.hip) */
hipError_t launch_export(const int64_t* off, const int32_t* st, int64_t nf, int64_t* h_off, int32_t* h_st,
                         hipStream_t s);
/* k_lpc<32> with the autocorrelation read from a.acf (flacmi_device_lpc_from_acf) */
hipError_t launch_lpc_from_acf(const LpcArgs& a, hipStream_t s);
/* path: 0 = int16 samples / sdot2, 1 = int32 samples / mad24, 2 = int64 arithmetic */
hipError_t launch_resid(const ResidArgs& a, int path, int residual_bytes, hipStream_t s);
/* k_resid_stream over the chunks of one length class (k_stream.hip): begin, every chunk's batch
 * kernel, then the list passes once */
bool stream_class_ok(const ResidArgs& cls, int path, int residual_bytes);
hipError_t launch_stream_class_begin(const ResidArgs& cls, hipStream_t s);
hipError_t launch_stream_class_batch(const ResidArgs& chunk, int64_t list_off, int64_t class_count, hipStream_t s);
hipError_t launch_stream_class_lists(const ResidArgs& cls, hipStream_t s);
hipError_t launch_expand_records(const int32_t* rec, int32_t rec_words, int32_t L, int64_t count,
                                 int32_t* out, hipStream_t s);
hipError_t launch_synth(void* dst, int32_t sample_bytes, int32_t bits, int64_t stride,
                        int64_t first_unit, int64_t n_units, int32_t len, uint64_t seed,
                        const int32_t* sintab, int32_t open8, hipStream_t s);
hipError_t launch_stats(const flacmi_unit_meta* meta, int64_t n_units, int32_t block_len,
                        int32_t tail_len, int64_t n_tail_units, int64_t* stats, hipStream_t s);

/* Stereo rows (k_stereo.hip): mid = (L + R) >> 1 in the input's element type and side = L - R in
 * int32 for every frame's row pair 2f, 2f + 1 of lr; len samples a row (tail_len for the last
 * frame when has_tail), elements from there to each output pitch zeroed.  Every row 16-byte
 * aligned, every pitch a multiple of 16 bytes. */
hipError_t launch_stereo_rows(const void* lr, int32_t sample_bytes, int64_t lr_stride, int64_t n_frames,
                              int32_t block_len, int32_t tail_len, int32_t has_tail, void* mid, int64_t mid_stride,
                              int32_t* side, int64_t side_stride, hipStream_t s);
/* Wasted bits (k_wasted.hip): wasted[u] = 0 for an all-zero unit, else min(ctz(OR of its samples),
 * sample_bits - 1), and out row u = in row u >> wasted[u]; len samples a row (tail_len for the last
 * n_tail_units units), nothing at or past a unit's length is read or written.  out may be in (with
 * the same pitch): units with wasted[u] == 0 are then not stored.  Every row 16-byte aligned,
 * every pitch a multiple of 16 bytes. */
hipError_t launch_wasted_rows(const void* in, int32_t sample_bytes, int64_t in_stride, int64_t n_units,
                              int32_t block_len, int32_t tail_len, int64_t n_tail_units, int32_t sample_bits,
                              void* out, int64_t out_stride, int32_t* wasted, hipStream_t s);
/* The exact Rice search (k_rice.hip, FLACMI_FLAG_RICE_SEARCH): one launch over every unit of an
 * analysis call, behind its last k_resid launch.  Units whose status is 0, or the reference's
 * ValueError at FLACMI_SITE_RICE_LOG_DOMAIN / FLACMI_SITE_RICE_NEG_SHIFT (which then become status 0),
 * get part_order, n_parts, coding_method, rice_bits, res_offset, res_len and rice_params[0 .. n_parts)
 * by the rule in include/flacmi.h; nothing else is written.  rmax <= 8. */
struct RiceArgs {
    flacmi_unit_meta* meta;  /* [n_units] */
    int32_t* rice_params;    /* [n_units][params_stride] */
    int64_t params_stride;
    const void* residual;    /* [n_units][residual_stride] u32 or u64 zig-zag rows, 16-byte aligned */
    int64_t residual_stride;
    int64_t n_units, n_tail_units;
    int32_t block_len, tail_len;
    int32_t rmin, rmax;
    int32_t mode;            /* FLACMI_MODE_RICE_ONLY: a rescued unit's predictor order is rice_order */
    int32_t rice_order;
    int32_t pitch;           /* set by the launcher: partitions the LDS tables are laid out for, 2^rmax */
};
/* grid_cap: workgroups at most, 0 = the default */
hipError_t launch_rice_search(const RiceArgs& a, int residual_bytes, int grid_cap, hipStream_t s);
/* The subframe choice by exact written size (k_size.hip, FLACMI_FLAG_SIZE_CHOICE): one launch over
 * every unit of an analysis call, behind k_lpc and in place of k_resid and k_rice_search.  Every
 * unit's whole record, its rice_params and its zig-zag row are written by the rule in
 * include/flacmi.h; a unit whose LPC record carries a status gets that status and site. */
struct SizeArgs {
    const void* samples;     /* int16 or int32 rows, 16-byte aligned */
    int64_t stride;
    int32_t sample_bytes;
    int32_t block_len, tail_len;
    int64_t n_units, n_tail_units;
    int32_t L, q, mode;      /* FLACMI_MODE_REFERENCE or FLACMI_MODE_FIXED_ONLY */
    int32_t rmin, rmax;      /* rmax <= 8 */
    int32_t ss;              /* bits a warm-up sample of these units is written at */
    const int32_t* rec;      /* [n_units][rec_words] k_lpc's records (NULL in fixed-only mode) */
    int32_t rec_words;
    flacmi_unit_meta* meta;  /* [n_units] */
    int32_t* rice_params;    /* [n_units][params_stride] */
    int64_t params_stride;
    void* residual;          /* [n_units][residual_stride] u32 or u64, 16-byte aligned rows */
    int64_t residual_stride;
    int64_t* fixed_sums;     /* optional [n_units][5]: each fixed candidate's bits, -1 when not eligible */
    int64_t* lpc_sums;       /* optional [n_units][32]: each LPC candidate's, 0 at and past L */
    int32_t pitch;           /* set by the launcher: 2^rmax */
};
/* dynamic LDS of k_size_choice for a call (the Rice tables, the best parameters, the candidate's
 * taps, the unit's record and its samples) */
size_t size_choice_lds(int block_len, int sample_bytes, int rec_words, int rmax);
/* grid_cap: workgroups at most, 0 = the default */
hipError_t launch_size_choice(const SizeArgs& a, int residual_bytes, int grid_cap, hipStream_t s);
/* a.choice[f] from the four candidates' sizes (after k_sub_kinds in the fallback mode) */
hipError_t launch_stereo_choose(const FrameArgs& a, hipStream_t s);

/* (a.sub_kind set: k_sub_kinds first; a.choice set: over the 4 n_frames candidates, then
 * k_stereo_choose,) frame sizes + exclusive scan into a.offsets; bsum:
 * frame_scan_blocks(n_frames) words */
hipError_t launch_frame_sizes(const FrameArgs& a, int64_t* bsum, hipStream_t s);
int64_t frame_scan_blocks(int64_t n_frames);
hipError_t launch_pack(const FrameArgs& a, hipStream_t s);
hipError_t launch_decode(DecodeArgs a, hipStream_t s);
hipError_t launch_index(const IndexArgs& a, hipStream_t s);
/* grid_cap: workgroups (of 64 frames) at most, 0 = the default */
hipError_t launch_frame_info(const InfoArgs& a, int grid_cap, hipStream_t s);
int64_t index_scan_groups(int64_t n_tiles);
hipError_t launch_pcm(const PcmArgs& a, hipStream_t s);
/* clears a.status [n_frames] and a.width, then one workgroup per unit; sample_bytes 2 or 4 */
hipError_t launch_units(const UnitsArgs& a, int32_t sample_bytes, hipStream_t s);
hipError_t launch_planar(PlanarArgs a, int32_t elem, hipStream_t s);

hipError_t launch_selftest(int32_t which, const double* x, double* out, int32_t* status, int64_t n,
                           const double* log2thr, hipStream_t s);

}  // namespace flacmi
