/*
 * flacmi.h — C-ABI of the MI355X FLAC encode-analysis library (libflacmi.so).
 *
 * This is the drop-in boundary for turlando/flac-py's per-block analysis hot path.
 * flac-py has no FFI layer of its own; the interface this library replaces is the
 * Python function triple called once per (block, channel) from encode():
 *
 *   encode_subframe_fixed(samples)                       flac/encoder.py:331-359
 *   encode_subframe_lpc(samples, lpc_order, precision)   flac/encoder.py:362-420
 *     (tukey 423-440, autocorrelation 443-450, levinson_durbin 453-479,
 *      quantize_lpc_coefficients 482-534, prediction_residual 537-548)
 *   the fixed-vs-LPC choice on sum(|residual|)           flac/encoder.py:133-157
 *   encode_residual(residual, block_size, sample_size,
 *                   predictor_order, partition_order_range)  flac/encoder.py:632-760
 *     (called by the writer at flac/encoder.py:588 and :608)
 *
 * One call analyses a whole batch of independent "units" (one unit = one channel of
 * one block) and returns, per unit, exactly the fields of the reference's
 * SubframeHeader / SubframeFixed / SubframeLPC / Residual / RicePartition values
 * (flac/common.py:286-309, 334-361, 378-420), bit-identical.  Where the reference
 * would raise a Python exception the unit's `status` names the exception class and
 * `site` names the raising statement (see flacmi_status / flacmi_site).
 *
 * Conventions: plain C types, caller-owned buffers, return 0 on success or a
 * negative flacmi_error; flacmi_last_error() describes the last failure of the
 * calling thread.  A context is bound to one HIP device and is not thread-safe;
 * use one context per host thread.  The *_device entry points take device pointers
 * and enqueue on the given hipStream_t (passed as void*), returning without a host
 * synchronisation; the *_host entry points take host pointers and are synchronous.
 * The *_device calls of one context share its scratch buffers (LPC records, retry and
 * pack lists, decoder state): issue them on one stream, or make each call's stream
 * wait for the previous call's work, never concurrently on two streams.
 */
#ifndef FLACMI_H
#define FLACMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: in the default (pruning) mode meta.lpc_order / meta.lpc_sum of a unit whose LPC
      candidates provably lose read FLACMI_LPC_PRUNED, and stats word 80 no longer folds
      lpc_sum (round 3); version 1 callers read exact LPC fields there
   3: flacmi_frame_params.reserved0 carries the frame flags (FLACMI_FRAME_FALLBACK) and a value
      with unknown bits is refused; version 2 callers passed 0 there and see no change
   4: flacmi_frame_params.reserved[1] is the stereo mode (enum flacmi_stereo_mode) and any value
      but 0 and 1 is refused; flacmi_stereo_rows_device is new; version 3 callers passed 0 there
      and see no change
   5: flacmi_params.reserved[1] takes FLACMI_FLAG_LPC_SIGN (the corrected LPC predictor sign, off by
      default); version 4 callers never set bit 2 there and see no change
   6: the stream analysis (flacmi_frame_info_device, flacmi_info_stream_host).  Added since, at
      the same version (no struct changes size): flacmi_wasted_rows_device, FLACMI_FRAME_WASTED in
      flacmi_frame_params.reserved0, and flacmi_decode_params.reserved0 carries the decode flags
      (FLACMI_DECODE_WASTED_SPEC); a value with unknown bits is refused, callers that passed 0 there
      see no change; FLACMI_FLAG_RICE_SEARCH in flacmi_params.reserved[1] (callers never set bit 8
      there and see no change); FLACMI_FLAG_SIZE_CHOICE in flacmi_params.reserved[1], with the written
      sample width in flacmi_params.reserved[2] (callers never set bit 16 there, passed 0 in
      reserved[2], and see no change) */
#define FLACMI_ABI_VERSION 6
#define FLACMI_MAX_LPC_ORDER 32      /* EncoderParameters: lpc_order.stop <= 33 (encoder.py:42) */
#define FLACMI_MAX_BLOCK 65535       /* largest block the reference writes (encoder.py:249-253, 16-bit uncommon
                                        code); analysis returns FLACMI_E_UNSUPPORTED where a block's
                                        workgroup staging exceeds LDS (above ~16K samples) */
#define FLACMI_MAX_RICE_ORDER 15     /* 4-bit partition-order field (encoder.py:767) */
#define FLACMI_LPC_REC_WORDS(L) (2 + (L) + ((L) * ((L) + 1)) / 2)

/* ---- return codes (API level) ------------------------------------------------ */
enum flacmi_error {
    FLACMI_OK = 0,
    FLACMI_E_INVALID = -1,       /* bad argument (shape, range, alignment) */
    FLACMI_E_HIP = -2,           /* HIP runtime error */
    FLACMI_E_UNSUPPORTED = -3,   /* shape this build does not handle (see flacmi_last_error) */
    FLACMI_E_NOMEM = -4,
};

/* ---- per-unit status: the Python exception the reference would raise ---------- */
enum flacmi_status {
    FLACMI_STATUS_OK = 0,
    FLACMI_STATUS_ZERO_DIVISION = 1,  /* ZeroDivisionError */
    FLACMI_STATUS_ASSERTION = 2,      /* AssertionError */
    FLACMI_STATUS_VALUE_ERROR = 3,    /* ValueError */
    FLACMI_STATUS_OVERFLOW = 4,       /* OverflowError */
    FLACMI_STATUS_RESIDUAL_WIDE = 16, /* not a reference exception: chosen residual does not fit
                                         the requested residual element width; re-run with 8 bytes */
};

/* ---- per-unit site: which reference statement raises ------------------------------ */
enum flacmi_site {
    FLACMI_SITE_NONE = 0,
    FLACMI_SITE_TUKEY = 1,           /* encoder.py:437  pi*i/nr with nr == 0 (4 <= n <= 7) */
    FLACMI_SITE_LEVINSON_DIV = 2,    /* encoder.py:469  lambda_ /= error, error == 0 */
    FLACMI_SITE_LEVINSON_POW = 3,    /* encoder.py:476  lambda_ ** 2 overflows */
    FLACMI_SITE_QUANT_CMAX = 4,      /* encoder.py:496  assert coef_max > 0.0 */
    FLACMI_SITE_QUANT_LOG2 = 5,      /* encoder.py:503  floor(log2(inf)) */
    FLACMI_SITE_QUANT_SHIFT = 6,     /* encoder.py:508  shift < shift_min */
    FLACMI_SITE_QUANT_ROUND_INF = 7, /* encoder.py:520/530 round(inf) */
    FLACMI_SITE_QUANT_ROUND_NAN = 8, /* encoder.py:520/530 round(nan) */
    FLACMI_SITE_LPC_EMPTY = 9,       /* encoder.py:404  min() of no candidate orders (-l 0) */
    FLACMI_SITE_CHOICE_TIE = 10,     /* encoder.py:157  fixed_size == lpc_size */
    FLACMI_SITE_RICE_NO_ORDER = 11,  /* encoder.py:669  no valid partition order */
    FLACMI_SITE_RICE_LOG_DOMAIN = 12,/* encoder.py:753  log2(0): partition sum is 0 */
    FLACMI_SITE_RICE_NEG_SHIFT = 13, /* encoder.py:758  1 << parameter, parameter < 0 */
    FLACMI_SITE_RESIDUAL_WIDTH = 14, /* not a reference site: see FLACMI_STATUS_RESIDUAL_WIDE */
    /* frame writer (flacmi_frame_sizes_device): statements of the reference's writer */
    FLACMI_SITE_CODED_NUMBER = 15,   /* coded_number.py:38  frame number needs more than 31 bits (ValueError) */
    FLACMI_SITE_LPC_PRECISION = 16,  /* encoder.py:619  assert precision - 1 != 0b1111 (AssertionError) */
    FLACMI_SITE_FRAME_SIZE = 17,     /* not a reference site: see FLACMI_STATUS_FRAME_TOO_LARGE */
};

/* frame writer status beyond the reference's exceptions */
#define FLACMI_STATUS_FRAME_TOO_LARGE 17 /* a frame of >= 2^28 bytes: this build does not pack it */

/* ---- analysis modes -------------------------------------------------------------- */
enum flacmi_mode {
    FLACMI_MODE_REFERENCE = 0,   /* fixed + LPC + choice + Rice, exactly as encode() does */
    FLACMI_MODE_FIXED_ONLY = 1,  /* fixed predictor + Rice only (BASELINE config 5; the
                                    reference's own -l 0 raises ValueError instead) */
    FLACMI_MODE_LPC_ONLY = 2,    /* encode_subframe_lpc alone (encoder.py:362-420): the best LPC
                                    candidate is the result, no fixed comparison, no Rice search
                                    (part_order = -1); its residual row is returned */
    FLACMI_MODE_RICE_ONLY = 3,   /* encode_residual alone (encoder.py:632-652): each row holds a
                                    residual at [reserved[0], len) for predictor order
                                    params.reserved[0]; only the Rice search runs */
};

enum flacmi_kind { FLACMI_KIND_FIXED = 0, FLACMI_KIND_LPC = 1 };

typedef struct flacmi_params {
    int32_t max_lpc_order;   /* L = lpc_order.stop - 1, 0..32 (lpc_order.start must be 0) */
    int32_t qlp_precision;   /* EncoderParameters.qlp_precision, 5..31 */
    int32_t rice_min;        /* rice_partition_order.start */
    int32_t rice_max;        /* rice_partition_order.stop - 1 (rice_max < rice_min: empty range) */
    int32_t mode;            /* flacmi_mode */
    int32_t reserved[3];     /* reserved[0]: predictor order in FLACMI_MODE_RICE_ONLY, else 0;
                                reserved[1]: flacmi_flags; reserved[2]: with FLACMI_FLAG_SIZE_CHOICE the
                                bits a warm-up sample is written at (0: batch.sample_bits), else 0 */
} flacmi_params;

/* params.reserved[1] bits */
enum flacmi_flags {
    /* compute every LPC candidate's exact sum(|r|) in FLACMI_MODE_REFERENCE (meta.lpc_order /
     * lpc_sum always exact).  Without it the analysis may prune: see FLACMI_LPC_PRUNED. */
    FLACMI_FLAG_ALL_CANDIDATES = 1,
    /* diagnostic: prune with the partial-sum tiers alone (no sign-correlation bound), so a
     * test reaches the tier decisions on data the bound already settles */
    FLACMI_FLAG_TIERS_ONLY = 2,
    /* the corrected LPC predictor sign: the analysis computes what the reference would if its
     * levinson_durbin (encoder.py:453-479) ended with `return [-c for c in coefs[1:]]`, i.e. the
     * predictor and not its negation.  The quantiser (encoder.py:482-534) runs on the negated
     * floats (its clamp is asymmetric, so the result is not the negated default record);
     * coef_max, the shift, every exception site, the ([], 0) negative-shift branch, the order
     * choice, the fixed/LPC comparison with its tie, the Rice search and the writers are
     * unchanged.  Honoured in FLACMI_MODE_REFERENCE and FLACMI_MODE_LPC_ONLY by every entry point
     * that takes flacmi_params; with FIXED_ONLY or RICE_ONLY the call fails with
     * FLACMI_E_INVALID.  The mode never prunes: meta.lpc_order / lpc_sum are exact,
     * FLACMI_LPC_PRUNED never appears and meta.lpc_tiers is 0 (0x101, one exact pass, on the units
     * k_resid_stream's list kernel takes, as with FLACMI_FLAG_ALL_CANDIDATES).  The reference decoder and
     * flacmi_decode_* read the LPC subframes it writes as they are. */
    FLACMI_FLAG_LPC_SIGN = 4,
    /* the exact Rice search (off by default; with it clear every byte, status, field and launch is as
     * without it).  The reference's find_rice_parameter (encoder.py:730-753) takes
     * floor(log2(sum / len)): no value when a partition's zig-zag sum is 0 (FLACMI_SITE_RICE_LOG_DOMAIN),
     * negative when the mean is below 1 (FLACMI_SITE_RICE_NEG_SHIFT), 31 (the 5-bit escape code) for a
     * mean >= 2^31 (the TODO at encoder.py:751), and not the minimum; rice_partitions evaluates every
     * candidate order before it chooses, so one near-silent stretch of n >> rice_max samples fails the
     * unit.  The mode replaces the estimate with the parameter that makes each partition smallest.
     * For a unit of n samples whose zig-zag residual is z = row[P .. n) (P = meta.res_offset where the
     * analysis succeeded, meta.order on a rescued unit, params.reserved[0] in FLACMI_MODE_RICE_ONLY):
     *   candidate orders  o in [rice_min, rice_max] with n % 2^o == 0 and (n >> o) > P
     *                     (encoder.py:664-667); with none the unit keeps FLACMI_SITE_RICE_NO_ORDER
     *   partitions        partition 0 has (n >> o) - P values, the others n >> o
     *                     (split_samples_in_partitions)
     *   partition cost    c_p(k) = sum_i (z_i >> k) + (1 + k) len_p  (sum of rice_size, encoder.py:756-760);
     *                     c4_p = min over k in 0..14, c5_p = min over k in 0..30, the parameter being
     *                     the smallest k that reaches the minimum
     *   written bits      W4(o) = sum_p (4 + c4_p), W5(o) = sum_p (5 + c5_p)
     *   walk              o ascending, method 4 before method 5: the first strictly smallest W wins.
     *                     So coding_method == 5 iff some parameter exceeds 14 (the invariant of
     *                     encode_residual, encoder.py:648-650), and no parameter exceeds 30.
     * Written: meta.part_order, n_parts, coding_method, res_offset = P, res_len = n - P,
     * rice_params[0 .. n_parts) and meta.rice_bits in the reference's estimate convention (W + 4 n_parts
     * for method 4, W + 3 n_parts + #{k_p > 14} for method 5: the frame writer's size of the residual
     * is W); nothing else of the record, no residual element, no rice_params word at or past n_parts.
     * Units: those whose status is 0, and those whose status is FLACMI_STATUS_VALUE_ERROR at
     * FLACMI_SITE_RICE_LOG_DOMAIN or FLACMI_SITE_RICE_NEG_SHIFT, which become status 0, site 0 (the
     * analysis has written their residual row and their kind, order, shift and coefs); every other
     * status is left alone (FLACMI_STATUS_RESIDUAL_WIDE: the caller's redo on 8-byte rows carries the
     * flag).  It is an analysis flag: every entry point that takes flacmi_params honours it in
     * FLACMI_MODE_REFERENCE, FIXED_ONLY and RICE_ONLY (the stereo mode's candidates and the wasted
     * mode's shifted units included); with FLACMI_MODE_LPC_ONLY, which has no Rice step, or with
     * rice_max > 8 (the FLAC subset bound) the call fails with FLACMI_E_INVALID before any launch.
     * One more kernel (k_rice_search) runs behind the analysis kernels. */
    FLACMI_FLAG_RICE_SEARCH = 8,
    /* the subframe choice by exact written size (off by default; with it clear every byte, status,
     * field and launch is as without it).  The reference picks the fixed order (encoder.py:350-352),
     * the LPC order (:398-404) and the subframe type (:135-157) by sum |r|, which ignores what an
     * order costs; the TODO in encode() (:104-118) wants "a reliable way of determining the size of
     * subframe structures".  The mode replaces those three statements and nothing else.  For a unit
     * of n samples written at ss bits (ss = params.reserved[2], or batch.sample_bits when that is 0:
     * batch.sample_bits only bounds the data, the stream may be wider):
     *   candidates   in this order: the fixed orders 0..4 (order 0 alone when n <= 4, :334); in
     *                FLACMI_MODE_REFERENCE then the LPC orders 1..L with the quantised coefficients
     *                and shift of the analysis' record for that order (so FLACMI_FLAG_LPC_SIGN is
     *                honoured as without the mode); FLACMI_MODE_FIXED_ONLY has the fixed ones only
     *   eligible     a candidate of predictor order P with a partition order (some o in
     *                [rice_min, rice_max] with n % 2^o == 0 and (n >> o) > P, :664-667) that, if LPC,
     *                is not in the quantiser's negative-shift branch (the ([], 0) record, which the
     *                reference writes undecodably) and has qlp_precision != 16 (the writer's
     *                assertion, :619)
     *   size         bits = 8 + P ss + (LPC: 9 + P qlp_precision) + 6 + W, with W the written residual
     *                size of FLACMI_FLAG_RICE_SEARCH on the candidate's zig-zag residual (same walk,
     *                same parameter ties): exact whatever the residual row width of the call
     *   choice       the first strictly smallest bits in candidate order; no tie raises
     *                (FLACMI_SITE_CHOICE_TIE never appears).  With no eligible candidate the unit has
     *                FLACMI_STATUS_ASSERTION at FLACMI_SITE_RICE_NO_ORDER and, but for fixed_* / lpc_*,
     *                a zero record.
     * A unit whose LPC stage fails (the record's status: sites 1..9, FLACMI_SITE_LPC_EMPTY included)
     * keeps that status and site and a zero record: encode_subframe_lpc raises before any choice.
     * Every other unit has status 0, except that a chosen residual that does not fit 4-byte rows
     * gives FLACMI_STATUS_RESIDUAL_WIDE as without the mode (kind, order, shift, coefs and fixed_* /
     * lpc_* written; the caller's redo on 8-byte rows carries the flag).  Written: the whole record
     * of the chosen candidate (kind, order, shift, ncoefs, coefs, res_offset = P, res_len = n - P,
     * part_order, n_parts, coding_method, rice_bits in the estimate convention of
     * FLACMI_FLAG_RICE_SEARCH), rice_params[0 .. n_parts) and the zig-zag residual row.
     * fixed_order / lpc_order are the first smallest eligible candidate of each family and
     * fixed_sum / lpc_sum its bits (-1 for both with no eligible candidate; lpc_* 0 in
     * FLACMI_MODE_FIXED_ONLY); lpc_tiers is 0.  outputs.fixed_sums[u][k] and outputs.lpc_sums[u][j]
     * hold every candidate's bits, -1 where it is not an eligible candidate (lpc_sums 0 at and past L).
     * Needs FLACMI_FLAG_RICE_SEARCH (with its rice_max <= 8), FLACMI_MODE_REFERENCE or
     * FLACMI_MODE_FIXED_ONLY and reserved[2] in 0..33; anything else fails with FLACMI_E_INVALID before any
     * launch.  flacmi_encode_host / flacmi_encode_pipeline fill reserved[2] from
     * flacmi_frame_params.sample_size when it is 0, refuse another value, pass ss + 1 for the stereo
     * mode's side rows, and refuse the flag together with FLACMI_FRAME_WASTED (the written width is
     * then per unit: a follow-up).  One kernel (k_size_choice) runs behind k_lpc in place of the
     * residual kernels and k_rice_search. */
    FLACMI_FLAG_SIZE_CHOICE = 16,
};

/* meta.lpc_order and meta.lpc_sum of a unit whose LPC candidates were pruned: exact lower
 * bounds proved every candidate's sum(|r|) strictly above the best fixed sum, so the
 * reference's choice (encoder.py:135-157) is the fixed subframe and no tie is possible.
 * Everything the reference writes (kind, order, residual, Rice fields) is unaffected.  Runs
 * with outputs.lpc_sums, FLACMI_FLAG_ALL_CANDIDATES or FLACMI_FLAG_LPC_SIGN never prune. */
#define FLACMI_LPC_PRUNED (-1)

/* One batch of units.  Samples are planar: unit u occupies
 * samples[u*unit_stride .. u*unit_stride + len(u)).  Every unit has `block_len`
 * samples except the last `n_tail_units`, which have `tail_len` (the short last
 * block of a stream, one unit per channel).  Rows must be 16-byte aligned. */
typedef struct flacmi_batch {
    const void* samples;     /* int16 (sample_bytes 2) or int32 (sample_bytes 4) */
    int32_t sample_bytes;    /* 2 or 4 */
    int32_t sample_bits;     /* every sample fits a signed integer of this many bits (<= 8*sample_bytes) */
    int64_t unit_stride;     /* elements between consecutive units (flacmi_unit_stride: the pitch
                                the library itself lays rows out at) */
    int64_t n_units;
    int32_t block_len;       /* 1..FLACMI_MAX_BLOCK */
    int32_t tail_len;        /* length of the trailing units, 1..block_len (ignored if n_tail_units == 0) */
    int64_t n_tail_units;    /* 0..n_units */
} flacmi_batch;

/* Per-unit result.  Field names follow flac/common.py:
 *   kind/order        -> SubframeHeader.type_ = SubframeTypeFixed(order) | SubframeTypeLPC(order)
 *   warmup            -> samples[:order]  (not copied: the caller has the samples)
 *   shift/coefs/ncoefs-> SubframeLPC.shift / .coefficients (qlp precision is the parameter)
 *   residual          -> residual row [res_offset, res_offset + res_len), zig-zag encoded,
 *                        i.e. the concatenation of RicePartition.residual
 *   part_order/n_parts/coding_method/rice params -> Residual  */
typedef struct flacmi_unit_meta {
    int32_t status;          /* flacmi_status */
    int32_t site;            /* flacmi_site */
    int32_t kind;            /* flacmi_kind of the chosen subframe */
    int32_t order;           /* predictor order of the chosen subframe = len(warmup) */
    int32_t shift;           /* SubframeLPC.shift (0 for fixed) */
    int32_t ncoefs;          /* len(SubframeLPC.coefficients): order, or 0 in the negative-shift branch */
    int32_t res_offset;      /* first valid element of the residual row */
    int32_t res_len;         /* len(residual) */
    int32_t fixed_order;     /* best fixed order 0..4 */
    int32_t lpc_order;       /* best LPC order 1..L (0 in fixed-only mode, FLACMI_LPC_PRUNED if pruned) */
    int32_t part_order;      /* Residual.partition_order as chosen by rice_partitions */
    int32_t n_parts;         /* len(Residual.partitions) */
    int32_t coding_method;   /* RiceCodingMethod value: 4 or 5 */
    int32_t lpc_tiers;       /* diagnostic, the pruning decision: LPC candidate passes made | passes of the
                                path << 8.  16-bit stream kernel: quarter-block bound passes 1..4, then 5 =
                                the exact pass; int8-MFMA path: eighths 2..8 of exact partial sums (8 = every
                                tile), 0/8 when the sign-correlation bound decides (k_resid_sb included);
                                16-bit k_resid: 0/1 (sign bound decides) or 1/1 (the exact LPC pass).  0 where
                                no pruning runs (fixed-only, all-candidates, the 64-bit chains) */
    int64_t fixed_sum;       /* sum(|r|) of the best fixed residual */
    int64_t lpc_sum;         /* sum(|r|) of the best LPC residual (0 in fixed-only mode, FLACMI_LPC_PRUNED if pruned) */
    int64_t rice_bits;       /* size estimate of the chosen partitioning (encoder.py:714-727) */
    int32_t coefs[FLACMI_MAX_LPC_ORDER];
} flacmi_unit_meta;

typedef struct flacmi_outputs {
    flacmi_unit_meta* meta;  /* [n_units] */
    int32_t* rice_params;    /* [n_units][params_stride], RicePartition.parameter per partition */
    int64_t params_stride;   /* >= 2^rice_max + 1 */
    void* residual;          /* [n_units][residual_stride] uint32 or uint64 zig-zag residuals */
    int32_t residual_bytes;  /* 4 or 8 */
    int32_t reserved0;
    int64_t residual_stride; /* elements, >= block_len */
    /* optional intermediates (NULL to skip), used by parity tests */
    double* acf;             /* [n_units][33]  autocorrelation lags 0..L */
    int64_t* fixed_sums;     /* [n_units][5]   sum(|r|) for fixed orders 0..4 */
    int64_t* lpc_sums;       /* [n_units][32]  sum(|r|) for LPC orders 1..L */
    int32_t* lpc_records;    /* [n_units][FLACMI_LPC_REC_WORDS(32)] status/site, negmask, shifts, coefs */
} flacmi_outputs;

typedef struct flacmi_ctx flacmi_ctx;

/* ---- library / context ------------------------------------------------------------ */
int flacmi_abi_version(void);
const char* flacmi_last_error(void);
int flacmi_device_count(void);
flacmi_ctx* flacmi_create(int device);
void flacmi_destroy(flacmi_ctx* ctx);

/* ---- the hot path ---------------------------------------------------------------- */
/* Device pointers, enqueued on `stream` (hipStream_t). */
int flacmi_analyze_device(flacmi_ctx* ctx, const flacmi_batch* batch,
                          const flacmi_params* params, const flacmi_outputs* out,
                          void* stream);
/* Host pointers; copies in and out, synchronous. */
int flacmi_analyze_host(flacmi_ctx* ctx, const flacmi_batch* batch,
                        const flacmi_params* params, const flacmi_outputs* out);

/* ---- frame writer: FLAC frames from the analysis results -------------------------- */
/* The reference writes each frame on the host, bit by bit (encoder.py:87-165 frame loop;
 * put_frame_header :194-234 with coded_number.py:7-39 and crc.py:18-31; _put_subframe_header
 * :553-569; _put_subframe_fixed/_lpc :581-627; put_residual / put_rice_partition /
 * put_rice_int :765-806; padding + CRC-16 footer :159-163).  These entry points produce
 * the same bytes on the device: frame f of a batch holds the units
 * [f*channels, (f+1)*channels) (one subframe per channel, in channel order); the last
 * frame may be short (the batch's tail units).  Frames are byte-aligned and packed back
 * to back in `out` at frame_offsets[f] .. frame_offsets[f+1].
 *
 * Fallback subframes (FLACMI_FRAME_FALLBACK, off by default; with it off every byte and
 * status is the reference's).  The reference raises on much real audio (digital silence, a
 * constant or linear block, a Rice partition whose mean zig-zag value is below 1) and never
 * compares a subframe with its raw size: the TODO in encode() (encoder.py:104-125) wants
 * verbatim subframes and "a reliable way of determining the size" of a subframe.  The mode
 * replaces that TODO with the reference's own writers that nothing calls:
 * encode_subframe_verbatim (:323-328) and the CONSTANT / VERBATIM cases of _put_subframe_type
 * with _put_subframe_verbatim (:559-578); the size is the exact bit count the frame writer
 * already computes.  A unit (one channel of one block, n samples, stream sample size ss) is
 * escaped when
 *   - its analysis status is a reference exception (ZeroDivisionError, AssertionError,
 *     ValueError, OverflowError), or
 *   - it is an LPC subframe and the writer's precision assertion (encoder.py:619) would raise, or
 *   - its status is 0 and its exact subframe size is strictly greater than 8 + n * ss bits, or
 *   - its status is 0, its n samples are all equal and its exact subframe size is strictly greater
 *     than 8 + ss bits (the reference fails every such block; with FLACMI_FLAG_RICE_SEARCH it is a
 *     FIXED subframe whose all-zero residual costs one bit a sample).
 * An escaped unit whose n samples are all equal is written as CONSTANT (header 0 000000 0, the
 * value in ss bits: 8 + ss bits), any other as VERBATIM (header 0 000001 0, every sample in ss
 * bits, two's complement truncated as warm-up samples are: 8 + n * ss bits).  Not escaped, so
 * failing the frame as before: FLACMI_STATUS_RESIDUAL_WIDE (the caller's 8-byte redo still
 * happens), a block size or frame number that cannot be coded, FLACMI_STATUS_FRAME_TOO_LARGE
 * and the output capacity.
 *
 * Stereo decorrelation (FLACMI_STEREO_BEST in reserved[1], off by default; with it off every
 * byte, status and launch is as without it).  encode() writes Channels.L_R for every frame
 * (encoder.py:95; the reference's README: "Stereo decorrelation is not implemented yet"), while
 * its decoder undoes all four stereo assignments (decoder.py:111-122, :431-451).  The mode is
 * honoured by flacmi_encode_host and flacmi_encode_pipeline for channels == 2 and
 * sample_size <= 31.  A frame of n samples with L = channel 0, R = channel 1 has four candidate
 * signals: L and R (ss bits), M = (L + R) >> 1 (arithmetic shift; ss bits) and S = L - R
 * (ss + 1 bits).  Each is analysed as a unit exactly as a channel holding those samples is (the
 * reference's per-channel analysis never looks at the sample size): same parameters, pruning,
 * status and site.  A candidate's size is the exact bit count the frame writer writes for its
 * subframe, warm-up and raw samples at the candidate's own width w.  Without
 * FLACMI_FRAME_FALLBACK a candidate is not eligible when its status is a reference exception or
 * it is an LPC subframe and the precision assertion (encoder.py:619) would raise; with it an
 * escaped candidate (the rule above, against 8 + n * w) counts its CONSTANT / VERBATIM size,
 * 8 + w or 8 + n * w.  The assignments are walked in the order
 *   L_R (channel code 1: subframes L, R), L_S (8: L, S), S_R (9: S, R), M_S (10: M, S)
 * and the frame takes the first with the smallest sum of its two sizes among those whose two
 * candidates are both eligible; its header carries that code and its side subframe is written
 * at ss + 1 bits.  With no eligible assignment the frame fails with the status the L_R frame has
 * without the mode.  FLACMI_STATUS_RESIDUAL_WIDE on any candidate fails the frame with that status
 * (the redo with 8-byte residual rows still happens); the frame-level failures are unchanged.
 *
 * Wasted bits (FLACMI_FRAME_WASTED, off by default; with it off every byte, status and launch is as
 * without it).  The reference's SubframeHeader carries wasted_bits (common.py:309) and every
 * encoder path writes 0 (encoder.py:326, :556).  The mode is honoured by flacmi_encode_host and
 * flacmi_encode_pipeline, which own their device copy of the rows; the *_device frame entry points
 * have no free slot for the array and refuse the bit.  For a unit of n samples x_i at the
 * stream's sample size ss, with m the bitwise OR of all x_i in two's complement: w = 0 when
 * m == 0 (digital silence has no wasted bits, as in libFLAC), otherwise w = ctz(m) clamped to
 * ss - 1 (flacmi_wasted_rows_device, below).  The unit is analysed and written as the unit holding
 * x_i >> w (arithmetic shift, exact) at ss - w bits: same parameters, pruning, status, site,
 * FIXED / LPC choice and Rice search as a channel holding those samples (the reference's
 * per-channel analysis never looks at the sample size).  Its subframe header is 0 tttttt 0 when
 * w == 0, as without the mode, and 0 tttttt 1, w - 1 zero bits and a one when w > 0 (8 + w bits);
 * warm-up, CONSTANT and VERBATIM samples are written at ss - w bits.  With FLACMI_FRAME_FALLBACK a
 * unit is escaped when its exact size exceeds its own VERBATIM size 8 + w + n (ss - w), or, all
 * samples equal, its own CONSTANT size 8 + w + (ss - w); CONSTANT
 * writes x_0 >> w; every other fallback rule is unchanged.  Every frame of such a batch goes
 * through the general writer.  It composes with FLACMI_FRAME_FALLBACK, FLACMI_MODE_FIXED_ONLY and
 * FLACMI_FLAG_LPC_SIGN; together with FLACMI_STEREO_BEST the call returns FLACMI_E_INVALID (a
 * follow-up).  batch.sample_bits stays an upper bound: kernel dispatch is unchanged.  STREAMINFO
 * is unchanged.  A decoder reads such a stream with FLACMI_DECODE_WASTED_SPEC (the reference's own
 * decoder cannot). */
enum flacmi_stereo_mode {
    FLACMI_STEREO_OFF = 0,
    FLACMI_STEREO_BEST = 1,
};
enum flacmi_frame_flags {
    FLACMI_FRAME_FALLBACK = 1,
    FLACMI_FRAME_WASTED = 4, /* not 2: callers and tests/test_gpu_fallback.py rely on bit 1 being refused */
};
/* per-unit decision of the fallback mode (sub_kind[u]) */
enum flacmi_sub_kind {
    FLACMI_SUB_ANALYSED = 0, /* the FIXED / LPC subframe of the analysis */
    FLACMI_SUB_CONSTANT = 1,
    FLACMI_SUB_VERBATIM = 2,
};
typedef struct flacmi_frame_params {
    int32_t channels;        /* units per frame, 1..8 (encode()'s channels) */
    int32_t sample_size;     /* bits per warm-up sample in the stream (encode()'s sample_size), 1..32 */
    int32_t qlp_precision;   /* SubframeLPC.precision (EncoderParameters.qlp_precision) */
    int32_t reserved0;       /* enum flacmi_frame_flags bits (the name predates them); any other bit: FLACMI_E_INVALID */
    int64_t first_frame;     /* coded number of the batch's first frame (block index, encoder.py:97) */
    int64_t reserved[2];     /* reserved[0]: with FLACMI_FRAME_FALLBACK, for the *_device entry points, a device
                                pointer to int32_t sub_kind[n_units] (flacmi_sub_kind) that
                                flacmi_frame_sizes_device writes and flacmi_pack_frames_device reads;
                                flacmi_encode_host / flacmi_encode_pipeline keep their own and ignore it.
                                reserved[1]: enum flacmi_stereo_mode, honoured by flacmi_encode_host and
                                flacmi_encode_pipeline (channels == 2, sample_size <= 31); the *_device entry
                                points, whose caller owns a 2-units-a-frame layout, refuse a non-zero mode;
                                any other value: FLACMI_E_INVALID */
} flacmi_frame_params;

/* Frame sizes and their exclusive prefix sums (device pointers, enqueued on `stream`).
 * frame_offsets[n_frames + 1] receives byte offsets (frame_offsets[n_frames] = total);
 * frame_status[n_frames] receives 0, or (site << 16) | status of the first subframe (in
 * channel order) the reference would fail on while analysing or writing the frame; such
 * a frame gets size 0 and is not written.  meta / rice_params are analyze outputs for the
 * same batch; n_frames = ceil(n_units / channels). */
int flacmi_frame_sizes_device(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_frame_params* fp,
                              const flacmi_unit_meta* meta, const int32_t* rice_params, int64_t params_stride,
                              int64_t* frame_offsets, int32_t* frame_status, void* stream);
/* Write every frame with status 0 into out[frame_offsets[f] ..) (device pointers).  The
 * residual rows are the analyze outputs (zig-zag u32 or u64 rows, residual_bytes 4 or 8).
 * out must hold frame_offsets[n_frames] bytes (checked on the device against out_capacity;
 * on overflow nothing is written and frame_status[0] is set to FLACMI_STATUS_FRAME_TOO_LARGE). */
int flacmi_pack_frames_device(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_frame_params* fp,
                              const flacmi_unit_meta* meta, const int32_t* rice_params, int64_t params_stride,
                              const void* residual, int32_t residual_bytes, int64_t residual_stride,
                              const int64_t* frame_offsets, int32_t* frame_status, uint8_t* out,
                              int64_t out_capacity, void* stream);
/* Host form of analyze + frame sizes + pack (synchronous): host samples in; frame_offsets
 * [n_frames + 1] and frame_status [n_frames] out.  The frame bytes stay in a context
 * buffer until flacmi_encode_fetch copies them (frame_offsets[n_frames] bytes) to the host. */
int flacmi_encode_host(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_params* params,
                       const flacmi_frame_params* fp, int64_t* frame_offsets, int32_t* frame_status);
int flacmi_encode_fetch(flacmi_ctx* ctx, uint8_t* out, int64_t bytes);

/* The mid and side rows of a two-channel batch (the stereo mode's first step; device pointers,
 * enqueued on `stream`): rows 2f and 2f + 1 of `lr` are the left and right channel of frame f
 * (lr->n_units even; int16 or int32 rows; a short last frame has n_tail_units == 2).  mid row f
 * receives (L + R) >> 1 (arithmetic shift, computed without the 33rd bit) in lr's element type
 * at a pitch of mid_stride elements, side row f receives L - R as int32 at a pitch of
 * side_stride elements (for 32-bit inputs the difference wraps; the stereo mode stops at 31).
 * Elements from the frame's length up to each pitch are written as 0.  Every row must be 16-byte
 * aligned, every pitch a multiple of 16 bytes and at least block_len elements. */
int flacmi_stereo_rows_device(flacmi_ctx* ctx, const flacmi_batch* lr, void* mid, int64_t mid_stride,
                              int32_t* side, int64_t side_stride, void* stream);

/* The wasted bits of every unit of a batch and the units without them (device pointers, enqueued
 * on `stream`).  FLAC lets a subframe declare k wasted bits: the k low bits that are zero in every
 * sample of the block, shifted out before prediction and shifted back in by the decoder; the
 * reference's SubframeHeader carries the field (common.py:309) and each of its encoder paths writes
 * 0 (encoder.py:326, :556).  The rule, for a unit of n samples x_i of in->sample_bits bits (int16
 * or int32 rows; the last n_tail_units units hold tail_len samples): with m the bitwise OR of all
 * x_i in two's complement, w = 0 when m == 0 (digital silence has no wasted bits, as in libFLAC),
 * otherwise w = ctz(m), clamped to sample_bits - 1.  wasted[u] receives w and row u of out_rows
 * (in's element type, a pitch of out_stride elements) receives x_i >> w (arithmetic shift, exact):
 * the unit a subframe of width sample_bits - w is analysed and written from.  Nothing at or past a
 * unit's length is read or written.  out_rows may equal in->samples (out_stride then equals
 * in->unit_stride): the rows are shifted in place and a unit with w == 0 is not stored, so a
 * batch without wasted bits costs one read of its samples; any other overlap is undefined.  Every
 * row must be 16-byte aligned, every pitch a multiple of 16 bytes and at least block_len elements.
 * This is the first step of FLACMI_FRAME_WASTED, which the host entry points run in place on
 * their own copy of the rows. */
int flacmi_wasted_rows_device(flacmi_ctx* ctx, const flacmi_batch* in, void* out_rows, int64_t out_stride,
                              int32_t* wasted, void* stream);

/* Pipelined host encode (SURVEY §8d end-to-end; the reference's encode() loop plus its
 * writer, encoder.py:87-165, 765-806): host sample rows in, FLAC frame bytes out, the batch
 * cut into sub-batches of units_per_batch units (a multiple of channels) with two in
 * flight: the copy of sub-batch k+1 to the device and its analysis overlap the frame
 * writing and the copy back of sub-batch k.  The caller's sample rows and `out` are
 * page-locked in place for the call (hipHostRegister) so both copies are DMA at PCIe rate.
 * Buffers the caller already page-locked with flacmi_host_register are used as they are
 * (no per-call register / unregister: the way to stream many calls through the same
 * buffers).
 * out receives the frames back to back; frame_offsets[n_frames + 1] their byte offsets and
 * frame_status[n_frames] as flacmi_frame_sizes_device (a failing frame has no bytes).
 * FLACMI_E_NOMEM if the frames exceed out_capacity (frame_offsets then hold the sizes of
 * the sub-batches written so far).  timing (optional) receives per-step times. */
typedef struct flacmi_encode_timing {
    double wall_ms;        /* the whole call */
    double h2d_ms;         /* sum over sub-batches of each step's own duration (HIP events): */
    double analyze_ms;     /*   host -> device sample copy, analysis (k_lpc + k_resid), */
    double sizes_ms;       /*   frame sizes + scan, frame writing (k_pack32 / k_pack), */
    double pack_ms;        /*   device -> host frame copy; the steps of different */
    double d2h_ms;         /*   sub-batches overlap in wall time */
    double register_ms;    /* hipHostRegister / Unregister of the caller's buffers */
    int64_t sub_batches;
    int64_t bytes_in;      /* sample bytes copied to the device */
    int64_t bytes_out;     /* frame bytes copied back */
} flacmi_encode_timing;
int flacmi_encode_pipeline(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_params* params,
                           const flacmi_frame_params* fp, int64_t units_per_batch, uint8_t* out,
                           int64_t out_capacity, int64_t* frame_offsets, int32_t* frame_status,
                           flacmi_encode_timing* timing);

/* Page-lock a host range for the lifetime the caller chooses (hipHostRegister on the
 * context's device), so repeated flacmi_encode_pipeline / flacmi_analyze_host calls over
 * the same buffers copy at PCIe rate without paying the page-locking each call.  Replaces
 * nothing in the reference (its encode() has no device copies); the host-side analogue of
 * keeping a reused buffer (__main__.py:94-109 writes one output file per run).
 * FLACMI_E_HIP if the range cannot be locked (e.g. it overlaps a locked range). */
int flacmi_host_register(flacmi_ctx* ctx, void* ptr, size_t bytes);
int flacmi_host_unregister(flacmi_ctx* ctx, void* ptr);

/* Page-locked host memory owned by the caller until flacmi_host_free (hipHostMalloc on the
 * context's device): the staging rows and frame buffer a streaming caller fills and drains
 * batch after batch (flac_amd.encoder's encode paths), with no per-call page-locking.
 * NULL (flacmi_last_error) if it cannot be allocated.  flacmi_host_free takes a NULL ctx too
 * (memory that outlives its context). */
void* flacmi_host_alloc(flacmi_ctx* ctx, size_t bytes);
int flacmi_host_free(flacmi_ctx* ctx, void* ptr);

/* ---- decoder verifier (BASELINE config 5 round trip) ------------- */
/* Replaces the reference's frame decoder: decoder.py:111-130 get_frame, :133-190
 * get_frame_header (+ coded_number.py:45-70 decode), :192-245 field decoders, :267-344
 * get_subframe / get_subframe_header / get_subframe_type, :346-355 get_wasted_bits, :358-421
 * get_residual / get_rice_partition / get_rice_int, :431-498 decode_frame / decode_*_subframe
 * / _decode_prediction.  Frame f is the bytes stream[frame_offsets[f] .. frame_offsets[f+1]).
 * Per frame the device parses the header, every subframe and the footer, restores the
 * samples and (optionally) compares them with the batch they were encoded from.
 *
 * frame_status[f] = (site << 16) | status: the exception the reference decoder raises
 * (AssertionError / ValueError / EOFError, flacmi_decode_site names the statement), or a
 * verifier finding the reference does not check (FLACMI_STATUS_VERIFY: CRC-8 / CRC-16,
 * frame end, frame number, block size, sample mismatch).  frame_mismatch[f] counts the
 * samples that differ from `expect` (0 when expect is NULL).  Decoding is byte-exact to
 * the reference on every valid frame, with two documented choices: an L_R frame holds
 * dp->channels subframes (encoder.py:95 writes L_R whatever the channel count, so the
 * reference decoder cannot read back its own mono or 3+ channel streams), and, as in
 * decode_subframe, wasted bits are parsed but not shifted back in.  A third concerns 32-bit
 * streams with L_S / S_R / M_S stereo only: the side channel is read at 33 bits, the reference
 * restores it with unbounded integers, the device keeps every subframe's history as int32.  A
 * side-channel sample outside int32 therefore fails the frame with FLACMI_STATUS_VERIFY at
 * FLACMI_DSITE_SIDE_RANGE (samples_out is then unspecified for the frame) instead of decoding
 * it modulo 2^32; a 33-bit side channel whose samples all fit int32 decodes exactly.  (The
 * encoder's stereo mode stops at 31 bits and never writes such a frame.)  Everywhere else the
 * history is the reference's value modulo 2^32: frames whose subframe samples and predictions
 * fit int32, all that a conforming stream of up to 32 bits holds, decode exactly.
 *
 * Wasted bits as the format codes them (FLACMI_DECODE_WASTED_SPEC in dp->reserved0, off by
 * default; with it off every sample, status and frame end is as above).  A subframe whose header
 * ends in a set flag bit codes k wasted bits as k - 1 zeros and a one.  The reference reads them
 * wrongly twice: get_wasted_bits (decoder.py:346-355) returns the number of zeros, k - 1, and
 * decode_subframe never shifts the samples back (get_subframe drops the header).  With the flag
 * (a) wasted = zeros + 1, so the subframe's sample width is ss + (1 for a side channel) - wasted
 * (a width <= 0 keeps FLACMI_DSITE_ESCAPE_ZERO), and (b) every restored sample of the subframe is
 * s << wasted before the comparison with `expect`, before stereo recombination and before the
 * PCM range check.  The parse, and so the frame's end, differs between the two readings: the flag
 * reaches every pass that parses frames (the stream decoder's two passes and probes, the chain
 * walk through their ends, flacmi_frame_info_device / flacmi_info_stream_host, which then report
 * wasted_bits = k and sample_bits accordingly).  Any other bit of reserved0: FLACMI_E_INVALID. */
enum flacmi_decode_flags {
    FLACMI_DECODE_WASTED_SPEC = 1,
};
#define FLACMI_STATUS_EOF 5        /* EOFError: the frame runs past the end of the stream */
#define FLACMI_STATUS_VERIFY 18    /* verifier finding (not a reference exception) */
enum flacmi_decode_site {
    FLACMI_DSITE_SYNC = 32,          /* decoder.py:134  assert sync code */
    FLACMI_DSITE_BLOCK_SIZE_CODE,    /* :194  assert 0 < block-size code < 15 */
    FLACMI_DSITE_SAMPLE_RATE_CODE,   /* :213  assert sample-rate code < 15 */
    FLACMI_DSITE_CHANNELS_CODE,      /* :232  assert channel code <= 10 */
    FLACMI_DSITE_SAMPLE_SIZE_CODE,   /* :239  assert sample-size code != 3 */
    FLACMI_DSITE_RESERVED,           /* :141  assert reserved bit == 0 */
    FLACMI_DSITE_SUBFRAME_PAD,       /* :319  assert subframe padding bit == 0 */
    FLACMI_DSITE_SUBFRAME_TYPE,      /* :329-331  assert reserved subframe type */
    FLACMI_DSITE_LPC_PRECISION,      /* :302  assert precision != 0b1111 */
    FLACMI_DSITE_CODING_METHOD,      /* :394  ValueError: cannot read coding method */
    FLACMI_DSITE_PARTITIONS,         /* :363-364  assert block size / partition order */
    FLACMI_DSITE_ESCAPE_ZERO,        /* binary.py:131 sint(0): ValueError negative shift count (an escape width of 0; a sample
                                      * read at a width ss - wasted <= 0, which FIXED order 0 never does) */
    FLACMI_DSITE_NEG_SHIFT,          /* :496-497  ValueError: negative LPC shift in _decode_prediction */
    FLACMI_DSITE_PADDING,            /* :126  assert frame padding == 0 */
    FLACMI_DSITE_EOF,                /* binary.py:40  EOFError: the stream ends inside the frame */
    FLACMI_DSITE_CRC8,               /* verifier: header CRC-8 mismatch (crc.py:18-22) */
    FLACMI_DSITE_CRC16,              /* verifier: frame CRC-16 mismatch (crc.py:25-31) */
    FLACMI_DSITE_FRAME_END,          /* verifier: the frame does not end at frame_offsets[f+1] */
    FLACMI_DSITE_FRAME_NUMBER,       /* verifier: coded number != first_frame + f */
    FLACMI_DSITE_BLOCK_SIZE,         /* verifier: block size != the expected unit length / out_stride */
    FLACMI_DSITE_CHANNELS,           /* verifier: header channel count != dp->channels */
    FLACMI_DSITE_SAMPLES,            /* verifier: decoded samples differ from `expect` */
    FLACMI_DSITE_PCM_RANGE,          /* __main__.py:46  to_bytes: a sample does not fit the PCM width (OverflowError) */
    FLACMI_DSITE_SIDE_RANGE,         /* verifier: a 33-bit side-channel sample (32-bit L_S / S_R / M_S) outside int32 */
};
typedef struct flacmi_decode_params {
    int32_t channels;        /* subframes per frame (STREAMINFO channels), 1..8 */
    int32_t sample_size;     /* STREAMINFO sample size, used when the header defers to it, 4..32 */
    int64_t first_frame;     /* coded number expected for frame 0, or -1: not checked */
    int32_t check_crc;       /* 1: verify CRC-8 and CRC-16 (the reference reads them unchecked) */
    int32_t reserved0;       /* enum flacmi_decode_flags bits (the name predates them); any other bit: FLACMI_E_INVALID */
    int64_t reserved[2];
} flacmi_decode_params;
/* All pointers are device pointers; the work is enqueued on `stream`.  stream_bytes is the
 * readable size of `stream` (4-byte aligned base).  expect: NULL, or the batch whose unit
 * f*channels + c the subframe c of frame f must reproduce (block_len / tail_len /
 * n_tail_units give the expected block sizes).  samples_out: NULL, or int32 rows
 * [n_frames*channels][out_stride] (out_stride a multiple of 4, 16-byte aligned rows) that
 * receive the decoded samples; required when a frame uses L_S / S_R / M_S stereo. */
int flacmi_decode_frames_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                                const int64_t* frame_offsets, int64_t n_frames,
                                const flacmi_decode_params* dp, const flacmi_batch* expect,
                                int32_t* samples_out, int64_t out_stride, int32_t* frame_status,
                                int64_t* frame_mismatch, void* stream);

/* The same, and frame_end[n_frames] (device pointer, or NULL: exactly the call above)
 * receives per frame the byte offset after its CRC-16 footer, i.e. where the reference's
 * reader stands after get_frame (decoder.py:111-130), or -1 where the frame raised a
 * reference exception or was not parsed to its end (a FLACMI_DSITE_BLOCK_SIZE /
 * FLACMI_DSITE_CHANNELS finding).  The parse does not depend on frame_offsets[f + 1]; only
 * the FLACMI_DSITE_FRAME_END finding does, so a caller who does not know where frames end
 * proposes any end and reads the true one here. */
int flacmi_decode_frames_end_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                                    const int64_t* frame_offsets, int64_t n_frames,
                                    const flacmi_decode_params* dp, const flacmi_batch* expect,
                                    int32_t* samples_out, int64_t out_stride, int32_t* frame_status,
                                    int64_t* frame_mismatch, int64_t* frame_end, void* stream);

/* ---- stream decoder: .flac bytes in, interleaved PCM out ---------------------------- */
/* Replaces the reference's decode loop: decoder.py:46-55 samples() over get_frames
 * (:100-108), and cmd_decode's to_bytes loop (__main__.py:45-50).  The reference learns
 * where a frame starts by decoding every frame before it.  Here the device lists every
 * position that could start a frame (a "candidate"), decodes all of them at once, and the
 * host walks the chain of true frames through the decoded ends ("Stream
 * decoder").
 *
 * A byte offset p >= first_byte is a candidate iff the bytes at p pass every header check of
 * get_frame_header (decoder.py:133-185: 15-bit sync, block-size code 1..14, sample-rate code
 * != 15, channel code <= 10, sample-size code != 3, reserved bit 0; the coded number read as
 * following_bytes says, continuation prefixes unchecked), the header with its CRC-8 byte lies
 * inside stream_bytes, and the CRC-8 (crc.py:18-22) of the header matches. */
typedef struct flacmi_frame_candidate {
    int64_t offset;           /* byte offset of the sync code */
    int64_t coded_number;     /* frame or sample number (coded_number.py:45-70) */
    int32_t block_size;       /* samples per channel */
    int32_t header_bytes;     /* header length, CRC-8 byte included */
    int32_t channel_code;     /* 0..10 */
    int32_t sample_size_code; /* 0..7 except 3 */
} flacmi_frame_candidate;
/* Bytes of the stream one workgroup of the index kernel scans; tiles count from the 16-byte
 * boundary at or below stream_data.  For tests that place headers across tile edges. */
int32_t flacmi_index_tile_bytes(void);
/* Device pointers, enqueued on `stream`.  table[capacity] receives the candidates in strictly
 * ascending offset order; *count always receives the true count: when it exceeds capacity
 * the table holds the first `capacity` candidates and the caller retries with a larger
 * table (at most stream_bytes / 2 candidates exist). */
int flacmi_index_frames_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                               int64_t first_byte, flacmi_frame_candidate* table, int64_t capacity,
                               int64_t* count, void* stream);

/* One frame of decoded rows for flacmi_pcm_out_device: channel c's samples are
 * rows[c * stride .. c * stride + block_size) (device int32). */
typedef struct flacmi_pcm_frame {
    const void* rows;
    int64_t stride;
    int64_t first_sample;    /* samples per channel in the frames before it */
    int32_t block_size;
    int32_t reserved0;
} flacmi_pcm_frame;
enum flacmi_pcm_mode {
    FLACMI_PCM_PACKED = 0,   /* bytes_per_sample little-endian two's complement bytes per sample */
    FLACMI_PCM_RAW32 = 1,    /* int32 per sample, no range check (bytes_per_sample ignored) */
};
/* Interleave (decoder.py:52 zip(*samples)) and pack (__main__.py:46-50 to_bytes): sample t of
 * channel c of a frame goes to out[((first_sample + t) * channels + c) * B ..), B =
 * bytes_per_sample (1..4) or 4 in raw mode.  frame_status[f] = FLACMI_STATUS_OVERFLOW where a
 * sample does not fit 8 B signed bits (to_bytes raises OverflowError; the frame's bytes are
 * then unspecified), FLACMI_STATUS_FRAME_TOO_LARGE where the frame does not lie inside
 * out_capacity (nothing written), else 0.  Device pointers (out 4-byte aligned), enqueued
 * on `stream`. */
int flacmi_pcm_out_device(flacmi_ctx* ctx, const flacmi_pcm_frame* frames, int64_t n_frames,
                          int32_t channels, int32_t bytes_per_sample, int32_t mode, uint8_t* out,
                          int64_t out_capacity, int32_t* frame_status, void* stream);

/* The same frame list as the encoder's unit rows (k_units; the counterpart of the call above,
 * for a stream that is decoded and encoded again without its samples leaving the device).  The
 * frames follow one another without gaps, ordered by first_sample.  The unit timeline starts at
 * sample first_sample (frames wholly before it are skipped): sample s >= first_sample of channel
 * c goes to unit ((s - first_sample) / block_len) * channels + c, element
 * (s - first_sample) % block_len.  n_blocks whole blocks are written, then, when tail_len > 0, one
 * block of tail_len < block_len samples: n_units = (n_blocks + (tail_len > 0)) * channels rows of
 * int16 (sample_bytes 2) or int32 (4) at a pitch of unit_stride elements (flacmi_unit_stride, or
 * any multiple of 16 bytes that holds block_len; rows 16-byte aligned).  Every element of a
 * written unit from its length to the pitch is written as 0, a sample no frame holds as 0;
 * samples past the last unit are not read and nothing outside the n_units rows is written,
 * whatever the frame list holds.  frame_status[f] (n_frames words) = FLACMI_STATUS_OVERFLOW
 * where a sample of frame f that the call reads does not fit sample_size (4..32, at most
 * 8 * sample_bytes) bits two's complement (the frame's samples are then unspecified in the
 * units), else 0.  *width receives the maximum over the samples written of x >= 0 ? x : ~x: with
 * k its bit length, min(sample_size, max(2, k + 1)) is the flacmi_batch.sample_bits of the rows.
 * Device pointers, enqueued on `stream`. */
int flacmi_units_out_device(flacmi_ctx* ctx, const flacmi_pcm_frame* frames, int64_t n_frames,
                            int32_t channels, int64_t first_sample, int32_t block_len, int64_t n_blocks,
                            int32_t tail_len, int32_t sample_size, void* units, int32_t sample_bytes,
                            int64_t unit_stride, int32_t* frame_status, uint32_t* width, void* stream);

/* The frame lists of many streams as one padded planar buffer (k_planar; the third consumer of
 * the list, for a library of short streams whose samples stay on the device).  frames[n_frames]
 * is ordered by (stream, first_sample): reserved0 holds the frame's stream index 0 .. n_streams
 * - 1 and first_sample counts from that stream's first sample; a stream's frames follow one
 * another without gaps.  Sample t of channel c of stream s goes to
 * out[(s * channels + c) * pitch + t]: n_streams * channels rows of `elem` at a pitch of `pitch`
 * elements (a multiple of 16 bytes; out 16-byte aligned).
 *   FLACMI_PLANAR_INT16    frame_status[f] = FLACMI_STATUS_OVERFLOW where a sample of frame f
 *                          that the call reads does not fit 16 bits (the frame's samples are
 *                          then unspecified), else 0;
 *   FLACMI_PLANAR_INT32    the decoder's int32, no check (the FLACMI_PCM_RAW32 meaning);
 *   FLACMI_PLANAR_FLOAT32  (float)x * 2^-(sample_size - 1): the int32 rounded to nearest even,
 *                          then an exact power-of-two scale; sample_size is 4..32.
 * lengths (device, [n_streams], or NULL: every frame counts) cuts stream s at lengths[s]
 * samples.  Every element of every row from the stream's length (the end of its last frame,
 * or lengths[s]) to the pitch is written as 0, a sample no frame holds as 0, samples at or past
 * the pitch are not read, and nothing outside the n_streams * channels rows is written, whatever
 * the frame list holds.  Device pointers, enqueued on `stream`. */
enum flacmi_planar_elem { FLACMI_PLANAR_INT16 = 0, FLACMI_PLANAR_INT32 = 1, FLACMI_PLANAR_FLOAT32 = 2 };
int flacmi_planar_out_device(flacmi_ctx* ctx, const flacmi_pcm_frame* frames, int64_t n_frames,
                             int64_t n_streams, int32_t channels, const int64_t* lengths, int32_t sample_size,
                             int32_t elem, void* out, int64_t pitch, int32_t* frame_status, void* stream);

/* The walk from frame to frame over the candidate table and the first pass's results (plain
 * host code, no device: get_frames' loop, decoder.py:100-108, with each frame's end looked
 * up instead of reached by reading).  status[k] / frame_end[k] are candidate k's results from
 * flacmi_decode_frames_end_device with frame k proposed to end at candidate k + 1 (or
 * stream_bytes).  Start with w->pos = first_byte, n_chain = 0, state = FLACMI_WALK_RUN.
 * Each call appends chain frames until
 *   FLACMI_WALK_DONE    the stream's end, or an EOFError frame (silent, as get_frames): w->pos
 *                       is the offset after the last whole frame;
 *   FLACMI_WALK_STOPPED any other reference exception, or a frame that cannot be parsed to its
 *                       end: w->stop_status = (site << 16) | status, the frame at w->pos;
 *   FLACMI_WALK_PROBE   w->pos is no candidate (a true header whose CRC-8 byte is wrong, which
 *                       the reference reads unchecked, or whatever follows a frame), or its block
 *                       exceeds the first pass's rows: the caller decodes the one frame
 *                       [w->pos, stream_bytes), stores its status and end in w->probe_status /
 *                       w->probe_end and calls again (every probe moves w->pos on: a stream whose
 *                       headers mostly fail CRC-8 decodes correctly, one launch per frame);
 *   FLACMI_WALK_FULL    chain_capacity reached: call again with more room.
 * Candidates the walk never lands on are false syncs inside frame data. */
enum flacmi_walk_state { FLACMI_WALK_RUN = 0, FLACMI_WALK_DONE = 1, FLACMI_WALK_STOPPED = 2,
                         FLACMI_WALK_PROBE = 3, FLACMI_WALK_FULL = 4 };
typedef struct flacmi_chain_frame {
    int64_t offset, end;     /* the frame is bytes [offset, end) */
    int64_t candidate;       /* its index in the table, or -1: an inserted start */
    int32_t status;          /* first-pass (or probe) status word; 0: decoded rows are final */
    int32_t reserved0;
} flacmi_chain_frame;
typedef struct flacmi_walk {
    int64_t pos;
    int64_t n_chain;
    int32_t state;           /* flacmi_walk_state */
    int32_t stop_status;
    int32_t probe_status;
    int32_t reserved0;
    int64_t probe_end;
} flacmi_walk;
int flacmi_host_chain_walk(const flacmi_frame_candidate* table, int64_t n_candidates, const int32_t* status,
                           const int64_t* frame_end, int64_t stream_bytes, int32_t final_chunk,
                           flacmi_walk* w, flacmi_chain_frame* chain, int64_t chain_capacity);

/* One chunk of a stream, host bytes in, host PCM out (synchronous): copy in, index, decode
 * every candidate (pass 1, frame k proposed to end at candidate k + 1, rows k * channels ..
 * at the pitch of max_block_size, STREAMINFO's, or of the largest block a candidate declares
 * when that is 0), the walk, pass 2 (every chain frame whose pass-1 status was not 0, i.e. a
 * false candidate inside it, an inserted start or an oversized block, again with the
 * chain's own offsets into rows of their own pitch; its status is final), the PCM kernel,
 * copy out.  dp->first_frame is not checked (the reference never checks frame numbers);
 * with dp->check_crc = 0, the reference's behaviour, no CRC finding can occur; with 1 a
 * finding stops the stream at that frame like an exception, as FLACMI_DSITE_SIDE_RANGE does
 * with either setting.  The verifier's documented choices hold (above FLACMI_STATUS_EOF).
 *
 * data[0 .. bytes) is the chunk, frames start at first_byte; final_chunk = 0 says more bytes
 * follow, so a frame the chunk cuts off ends the call with res->consumed at its start (the
 * caller carries the tail over), where the final chunk ends silently as get_frames does.
 * pcm[pcm_capacity] receives the frames that fit whole; the first that does not ends the
 * call like a cut-off frame.  A frame whose samples overflow the PCM width stops the stream
 * with FLACMI_STATUS_OVERFLOW / FLACMI_DSITE_PCM_RANGE; the frames before it are delivered,
 * none of its own samples (the reference writes the frame's samples up to the failing one
 * before raising: the difference is frame-granular).  FLACMI_E_UNSUPPORTED when the
 * candidates' rows would exceed 4 GiB: pass a smaller chunk. */
typedef struct flacmi_stream_result {
    int64_t frames;          /* frames delivered */
    int64_t samples;         /* samples per channel delivered */
    int64_t pcm_bytes;       /* bytes written to pcm */
    int64_t consumed;        /* offset after the last delivered frame */
    int32_t status, site;    /* why the stream stopped: 0, 0 = it has not (end of chunk or stream) */
    int64_t candidates;      /* k_index's count */
    int64_t probes;          /* inserted starts and oversized blocks decoded one by one */
    int64_t pass2_frames;    /* chain frames decoded again */
    int64_t pcm_full;        /* 1: the call ended because the next frame does not fit pcm_capacity */
    int64_t reserved0;
} flacmi_stream_result;
int flacmi_decode_stream_host(flacmi_ctx* ctx, const uint8_t* data, int64_t bytes, int64_t first_byte,
                              const flacmi_decode_params* dp, int32_t max_block_size, int32_t final_chunk,
                              uint8_t* pcm, int64_t pcm_capacity, int32_t mode, int32_t bytes_per_sample,
                              flacmi_stream_result* res);

/* ---- batch decoder: many whole streams in one call, planar on the device ---------------- */
/* n_streams whole streams through the steps above, once: data holds their frame regions only
 * (magic and metadata stripped), stream s being data[seg_offsets[s] .. seg_offsets[s + 1]),
 * packed back to back (seg_offsets[0] = 0, ascending; an empty region is a stream of no frame).
 * One copy in, one index and one pass 1 over the whole buffer (every region's first byte joins
 * the candidates), the walk once per stream over its slice of the table with the region's end as
 * the stream's end, probes and pass 2 with that end as well.  Each stream decodes exactly as
 * flacmi_decode_stream_host decodes it alone with final_chunk = 1: a frame its region cuts off
 * ends it silently, whatever the next region's bytes would complete it to, and the stop of one
 * stream (results[s].status / site: 0, 0 = none) touches no other.  One dp for the call: the
 * streams share channels, sample_size, check_crc and the flags.  The rows and the frame list stay
 * in the context until its next stream, batch or recompress call.  FLACMI_E_UNSUPPORTED when
 * pass 1's rows would exceed 4 GiB (pass fewer streams), FLACMI_E_INVALID for n_streams < 1 or
 * seg_offsets that do not start at 0 or descend.
 *
 * flacmi_decode_batch_fetch then writes the kept frame list as planar rows (see
 * flacmi_planar_out_device: elem, pitch in elements, a multiple of 16 bytes and at least the
 * longest stream's samples) into out[n_streams][channels][pitch]: a device buffer, written on
 * `stream`, or with host_out != 0 host memory (synchronous; `stream` ignored).  With
 * FLACMI_PLANAR_INT16 a frame holding a sample outside 16 bits stops its stream there like
 * FLACMI_DSITE_PCM_RANGE in the stream decoder (the call waits for the kernel, and writes the
 * affected rows again): results[n_streams] (optional) receives the streams' final frames,
 * samples, consumed, status and site.  Every element from a stream's final length to the pitch
 * is 0.
 *
 * Ordering: flacmi_decode_batch_host is synchronous on the context's own stream.  A fetch into a
 * device buffer with FLACMI_PLANAR_INT32 or FLACMI_PLANAR_FLOAT32 only enqueues k_planar on
 * `stream`, and that kernel reads the context's rows: the caller must have synchronised `stream`
 * (or otherwise know the kernel finished) before the context's next stream, batch or recompress
 * call, which reuses or frees those rows on the context's stream without waiting for `stream`, and
 * before flacmi_destroy.  The FLACMI_PLANAR_INT16 and host_out fetches return with the rows
 * written. */
typedef struct flacmi_batch_stream_result {
    int64_t frames;          /* frames delivered */
    int64_t samples;         /* samples per channel delivered */
    int64_t consumed;        /* offset in data after the last delivered frame */
    int32_t status, site;    /* why the stream stopped: 0, 0 = it has not (its end, or a cut-off frame) */
    int64_t probes;          /* as flacmi_stream_result, this stream's */
    int64_t pass2_frames;
    int64_t reserved[2];
} flacmi_batch_stream_result;
typedef struct flacmi_batch_summary {
    int64_t candidates;      /* k_index's count over the whole buffer */
    int64_t frames;          /* frames delivered, all streams */
    int64_t max_samples;     /* the longest stream's samples per channel */
    int64_t probes, pass2_frames;
    int64_t reserved[3];
} flacmi_batch_summary;
int flacmi_decode_batch_host(flacmi_ctx* ctx, const uint8_t* data, const int64_t* seg_offsets, int64_t n_streams,
                             const flacmi_decode_params* dp, int32_t max_block_size,
                             flacmi_batch_stream_result* results, flacmi_batch_summary* summary);
int flacmi_decode_batch_fetch(flacmi_ctx* ctx, void* out, int64_t pitch, int32_t elem, int32_t host_out,
                              flacmi_batch_stream_result* results, void* stream);

/* ---- recompress: .flac bytes in, .flac frames out, the samples stay on the device ------- */
/* One chunk of a stream through the decoder above (steps copy in .. pass 2, same arguments:
 * first_byte, dp with check_crc and FLACMI_DECODE_WASTED_SPEC, max_block_size, final_chunk) and,
 * instead of the PCM kernel, through k_units into unit rows of block_len samples and
 * flacmi_encode_host's analysis and frame writer (params and fp as there: every flag and mode,
 * every refusal).  Only compressed bytes cross PCIe.
 *
 * The context keeps a carry: the fewer than block_len samples per channel behind the last whole
 * block, as int32 rows, which open the next call's first block.  restart != 0 discards the carry
 * and the block counter first (a new stream).  Block k of the stream (counted since the last
 * restart) is written with the coded number fp->first_frame + k.  The unit rows are int16 when
 * fp->sample_size <= 16, else int32; the frame bytes do not depend on that.
 *
 * A stopping frame is a decoder status (as flacmi_decode_stream_host reports it) or a sample
 * that does not fit fp->sample_size bits (FLACMI_STATUS_OVERFLOW at FLACMI_DSITE_PCM_RANGE): the
 * whole blocks that lie entirely before its first sample are encoded and delivered,
 * res->consumed is its offset, and the carry is dropped.  With final_chunk set and the stream
 * at its end the carry goes out as the short last block; a final call with bytes == first_byte
 * does the same.  FLACMI_E_INVALID, before any device work, for whatever flacmi_encode_host
 * refuses for the same params / fp, for block_len outside 1..FLACMI_MAX_BLOCK and for dp
 * disagreeing with fp on channels or sample_size.
 *
 * The new frames stay in a context buffer, as flacmi_encode_host leaves them:
 * flacmi_recompress_fetch copies frame_offsets [blocks_out + 1], frame_status [blocks_out] (as
 * flacmi_frame_sizes_device: a failing block has no bytes) and the frame_bytes bytes out. */
typedef struct flacmi_recompress_result {
    int64_t frames;          /* input frames consumed */
    int64_t samples;         /* samples per channel they hold */
    int64_t consumed;        /* offset after the last of them */
    int32_t status, site;    /* why the input stopped: 0, 0 = it has not */
    int64_t candidates, probes, pass2_frames; /* as flacmi_stream_result */
    int64_t blocks_out;      /* frames written by this call (failing ones included) */
    int64_t frame_bytes;     /* their bytes */
    int32_t carry;           /* samples per channel kept for the next call */
    int32_t sample_bits;     /* the measured flacmi_batch.sample_bits of the call's unit rows (0: none) */
    int64_t reserved[2];
} flacmi_recompress_result;
int flacmi_recompress_host(flacmi_ctx* ctx, const uint8_t* data, int64_t bytes, int64_t first_byte,
                           const flacmi_decode_params* dp, int32_t max_block_size, int32_t final_chunk,
                           int32_t restart, int32_t block_len, const flacmi_params* params,
                           const flacmi_frame_params* fp, flacmi_recompress_result* res);
int flacmi_recompress_fetch(flacmi_ctx* ctx, int64_t* frame_offsets, int32_t* frame_status, int64_t n_blocks,
                            uint8_t* out, int64_t bytes);

/* ---- stream analysis: what a .flac holds, frame by frame (flac-py README, known issue 3) -- */
/* The reference has no such tool ("It would be nice to have a tool providing information
 * about a FLAC file, as `flac -a` does").  k_frame_info walks a frame exactly as get_frame
 * does (decoder.py:111-130, :133-262, :267-421) and reports what it read instead of restoring
 * samples.  It takes frame starts only: the frame ends where the parse stops.
 *
 * status = (site << 16) | status from the decoder's catalogue (flacmi_decode_site), but only
 * the exceptions get_frame itself raises, and EOFError: a negative LPC shift is reported in
 * `shift`, not as FLACMI_DSITE_NEG_SHIFT (_decode_prediction raises that, after get_frame),
 * and no verifier finding exists here: both CRCs are always computed and reported beside the
 * stored ones, a mismatch is a fact of the stream.  The decoder's two documented choices hold
 * (above FLACMI_STATUS_EOF): an L_R frame holds dp->channels subframes, wasted bits are
 * counted, not applied.  Sample-rate code 11 reports 96000 (the reference's table lacks the
 * entry: common.py:149-161). */
typedef struct flacmi_frame_info {
    int64_t offset;            /* the frame's first byte (frame_offsets[f]) */
    int64_t end;               /* the byte after the CRC-16, or -1: the parse raised */
    int64_t coded_number;      /* coded_number.py:45-70 */
    int32_t status;            /* 0, or (site << 16) | status of the exception get_frame raises */
    int32_t block_size;
    int32_t blocking_strategy; /* 0 fixed, 1 variable */
    int32_t sample_rate;       /* Hz as decoder.py:157-167 yields it; 0: from STREAMINFO */
    int32_t sample_size;       /* bits; 0: from STREAMINFO */
    int32_t channel_code;      /* 0..7 independent channels - 1, 8 L_S, 9 S_R, 10 M_S */
    int32_t n_subframes;       /* subframes fully parsed */
    int32_t header_bytes;      /* CRC-8 byte included */
    int32_t crc8_stored, crc8_computed;   /* crc.py:18-22 over the header */
    int32_t crc16_stored, crc16_computed; /* crc.py:25-31 over [offset, end - 2); 0, 0 when end is -1 */
    int32_t padding_bits;      /* zero bits between the last subframe and the CRC-16 */
    int32_t reserved0;
} flacmi_frame_info;
enum flacmi_subframe_type { FLACMI_SUB_TYPE_CONSTANT = 0, FLACMI_SUB_TYPE_VERBATIM = 1, FLACMI_SUB_TYPE_FIXED = 2,
                            FLACMI_SUB_TYPE_LPC = 3 };
typedef struct flacmi_subframe_info {
    int64_t bit_offset;        /* of the subframe's padding bit, from the frame's first bit */
    int64_t bits;              /* the subframe's total size */
    int32_t type;              /* flacmi_subframe_type */
    int32_t order;             /* predictor order (0 for CONSTANT / VERBATIM) */
    int32_t wasted_bits;
    int32_t sample_bits;       /* the width read: stream size + decorrelation bit - wasted */
    int32_t precision;         /* LPC: coefficient width in bits (the field + 1), else 0 */
    int32_t shift;             /* LPC: signed, as read; else 0 */
    int16_t coefficients[32];  /* LPC: the first `order`, the rest 0; all 0 otherwise */
    int32_t coding_method;     /* Rice parameter width: 4, 5, or 0 for none */
    int32_t partition_order;
    int32_t escaped_partitions;
    int32_t reserved0;
    int64_t residual_bits;     /* from the coding-method field to the last code */
    int64_t abs_sum;           /* sum |r| of the residual (what encode() compares, encoder.py:135-157) */
    int64_t constant_value;    /* CONSTANT only */
    int32_t partitions_stored; /* min(2^partition_order, part_stride) */
    int32_t reserved1;
} flacmi_subframe_info;
/* All pointers are device pointers; the work is enqueued on `stream` (stream_data 4-byte
 * aligned, readable up to the next multiple of 4 after stream_bytes).  frame_info[n_frames];
 * subframe_info rows [n_frames][dp->channels]: of frame f the first min(n_subframes,
 * dp->channels) records are written, the others left as they were (a header that declares
 * more channels than dp->channels has the further subframes parsed and counted only).
 * part_params[n_frames][dp->channels][part_stride] bytes (part_stride >= 0, NULL when 0): one
 * byte per partition, the Rice parameter, or 0x80 | width for an escaped partition; of a
 * subframe the first partitions_stored bytes are written, partitions at and beyond part_stride
 * are parsed and counted but not stored.  dp->first_frame and dp->check_crc are not used. */
int flacmi_frame_info_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                             const int64_t* frame_offsets, int64_t n_frames, const flacmi_decode_params* dp,
                             flacmi_frame_info* frame_info, flacmi_subframe_info* subframe_info,
                             uint8_t* part_params, int64_t part_stride, void* stream);

/* One chunk of a stream, host bytes in, host records out (synchronous), the sibling of
 * flacmi_decode_stream_host: copy in, k_index, k_frame_info over every candidate, the
 * candidates' records out, flacmi_host_chain_walk over their status / end (a
 * FLACMI_WALK_PROBE launches k_frame_info for the one offset), and the chain frames' records
 * gathered into the caller's arrays in stream order: frame_info[frame_capacity],
 * subframe_info[frame_capacity][dp->channels], part_params[frame_capacity][dp->channels]
 * [part_stride] (host pointers).  first_byte / final_chunk / consumed as in the decode call: a
 * frame the chunk cuts off ends the call with res->consumed at its start.  A frame that raises
 * stops the stream: res->status / site, and its own record is not delivered. */
typedef struct flacmi_info_result {
    int64_t frames;          /* frames delivered */
    int64_t consumed;        /* offset after the last delivered frame */
    int32_t status, site;    /* why the stream stopped: 0, 0 = it has not */
    int64_t candidates;      /* k_index's count */
    int64_t probes;          /* starts that were no candidate, parsed one by one */
    int64_t full;            /* 1: frame_capacity reached; call again from `consumed` */
    int64_t reserved0;
} flacmi_info_result;
int flacmi_info_stream_host(flacmi_ctx* ctx, const uint8_t* data, int64_t bytes, int64_t first_byte,
                            const flacmi_decode_params* dp, int32_t final_chunk, flacmi_frame_info* frame_info,
                            flacmi_subframe_info* subframe_info, uint8_t* part_params, int64_t part_stride,
                            int64_t frame_capacity, flacmi_info_result* res);

/* ---- stream statistics (reduced across GPUs with one RCCL all-reduce) ------------- */
#define FLACMI_STATS_WORDS 128
/* stats[0] units, [1] samples, [2] rice bits, [3] fixed units, [4] lpc units,
 * [5..9] fixed order histogram, [10..42] lpc order histogram (index 10+order-1... 41),
 * [48..63] partition order histogram, [64..79] status histogram, [80] checksum of the units'
 * (rice_bits, fixed_sum, kind, order): results that do not depend on LPC pruning; [81] units whose
 * LPC candidates were pruned (FLACMI_LPC_PRUNED) */
int flacmi_stream_stats(flacmi_ctx* ctx, const flacmi_unit_meta* d_meta, int64_t n_units,
                        int32_t block_len, int32_t tail_len, int64_t n_tail_units,
                        int64_t* d_stats, void* stream);

/* ---- the cross-GPU stats reduce without torch (SURVEY §8b flacmi_allreduce_stats) ----- */
/* One process (or host thread) per GPU.  Rank 0 makes an id with flacmi_comm_id and hands
 * its FLACMI_COMM_ID_BYTES to every rank over any out-of-band channel (a file, a socket,
 * MPI); each rank then calls flacmi_comm_init with the same id, the world size and its rank
 * (collective: every rank must call it).  RCCL (librccl.so.1, loaded on first use) runs
 * the all-reduce over xGMI.  Replaces the reference's nothing: flac-py is single-process;
 * the streams' statistics are the only cross-GPU exchange (encoder.py:81 writes no MD5). */
#define FLACMI_COMM_ID_BYTES 128
typedef struct flacmi_comm flacmi_comm;
/* 0 when RCCL loads here with every entry point the communicator uses (a local check, no id
 * or socket made): every rank runs it before rank 0 makes the id and all ranks enter the
 * collective flacmi_comm_init.  A failure inside ncclCommInitRank itself is not covered. */
int flacmi_comm_available(void);
int flacmi_comm_id(void* id_out);
int flacmi_comm_init(flacmi_ctx* ctx, int nranks, int rank, const void* id, flacmi_comm** out);
/* Sum of every rank's FLACMI_STATS_WORDS int64 words, in place (device pointer), enqueued
 * on `stream` (a stream of the communicator's context device). */
int flacmi_allreduce_stats(flacmi_comm* comm, int64_t* d_stats, void* stream);
int flacmi_comm_destroy(flacmi_comm* comm);

/* ---- row layout ------------------------------------------------------------------------ */
/* The unit pitch, in samples, at which this library lays out device rows (the *_host entry
 * points' mirrors, the encode pipeline's sub-batches) and which it recommends to callers of
 * the *_device entry points: the row rounded up to 16 bytes, plus 128 bytes when that is a
 * multiple of 4 KB.  k_lpc reads 64 rows at one offset per load instruction; at a 4 KB-multiple
 * pitch those lines fall into the same L2 sets and are fetched again.  A host
 * batch already at this pitch goes to the device as one linear copy.  No device needed. */
int64_t flacmi_unit_stride(int32_t block_len, int32_t sample_bytes);

/* ---- synthetic PCM (BASELINE configs 2-5) --------------------------------- */
/* Writes units [first_unit, first_unit + n_units) of the integer synthetic signal into
 * dst[(u - first_unit) * unit_stride ...]: sum of 3 DDS sinusoids + splitmix64 noise,
 * clipped to sample_bits; bit-identical to oracle/flac_oracle.c:oracle_synth_unit. */
int flacmi_synth_device(flacmi_ctx* ctx, void* dst, int32_t sample_bytes, int32_t sample_bits,
                        int64_t unit_stride, int64_t first_unit, int64_t n_units, int32_t len,
                        uint64_t seed, void* stream);
/* The same with open_eighths / 8 of the units (those whose hash byte is below open_eighths)
 * replaced by MA(1) near-white noise, whose LPC candidates tie the fixed order-0 sum within a
 * fraction of a percent: no bound decides them, so every candidate's exact sum is computed
 * (bench.py --open, the "undecided" workload).  Bit-identical to oracle_synth_unit_mix;
 * open_eighths = 0 is flacmi_synth_device. */
int flacmi_synth_mix_device(flacmi_ctx* ctx, void* dst, int32_t sample_bytes, int32_t sample_bits,
                            int64_t unit_stride, int64_t first_unit, int64_t n_units, int32_t len,
                            uint64_t seed, int32_t open_eighths, void* stream);

/* ---- device memory helpers (so hosts without a HIP binding can drive the device path) --- */
void* flacmi_device_alloc(flacmi_ctx* ctx, size_t bytes);
int flacmi_device_free(flacmi_ctx* ctx, void* ptr);
int flacmi_memcpy_h2d(flacmi_ctx* ctx, void* dst, const void* src, size_t bytes);
int flacmi_memcpy_d2h(flacmi_ctx* ctx, void* dst, const void* src, size_t bytes);
int flacmi_synchronize(flacmi_ctx* ctx);

/* ---- kernel timing (HIP events recorded on the stream each analyze call runs on) ----- */
/* Averages over the analyze calls since the last flacmi_timing_reset (up to 256 calls):
 * ms[0] k_lpc phase (autocorrelation + Levinson + quantisation), ms[1] k_resid phase
 * (residual sums + choice + Rice), ms[2] whole call, ms[3] number of calls averaged.
 * Synchronises on the recorded events; returns the number of values written. */
int flacmi_last_timing(flacmi_ctx* ctx, float* ms, int n);
int flacmi_timing_reset(flacmi_ctx* ctx);

/* ---- test and diagnostic knobs ---------------------------------------------------------- */
/* Process-wide knobs for A/B runs and tests, read from the environment once (the first time
 * any is used) and changed afterwards only through flacmi_set_knob, so no launch calls getenv
 * while another thread may change the environment.  Names: "FLACMI_OVERLAP" (analyze chunk
 * overlap: -1 round-aligned (default), 0 off, k > 1 equal chunks, -R R units per round),
 * "FLACMI_MF8_GRID" (cap on the int8-MFMA persistent grid, 0 = none), "FLACMI_STREAM_GENERIC"
 * (1 = the runtime-shape stream kernel for 4608-sample units), "FLACMI_DECODE_GENERIC" (1 =
 * every frame of flacmi_decode_frames_device through the general decoder kernel),
 * "FLACMI_PACK_GENERIC" (frame writer: 1 = every frame through the general writer kernel,
 * 2 = no ring-window writer (the one-window writer where a frame fits, else the general one),
 * 3 = the ring writer with 2048-value tiles on the ring the sample width ships with (2 KB
 * for samples of <= 16 bits, else 4 KB), 6 / 8 = the ring writer built for 256 / 128
 * threads, 7 = as 2 with the one-window writer on its 16 KB window only), "FLACMI_DECODE_LPC"
 * (0 = no second fast-decoder pass for LPC subframes: those frames go to the general decoder
 * kernel; default 1), "FLACMI_ENERGY_BOUND" (the stream kernel's pruning calls: 1 = prove LPC's
 * loss from the autocorrelation first, then, where that fails, for orders 2 .. L alone with
 * order 1 by a closed form on the fixed sums, then the partial-sum tiers (default); 0 = the
 * tiers alone; 2 = the first proof, then the exact sums; 3 = both proofs, then the exact sums;
 * 4 = the first proof, then the tiers; same results but for meta.lpc_tiers, and under 2 and 3
 * the exact LPC order and sum of a unit the tiers would have pruned),
 * "FLACMI_INFO_GRID" (cap on k_frame_info's grid in workgroups of 64 frames, 0 = the default
 * 2048; tests force a grid-stride loop with it).
 * FLACMI_E_INVALID for any other name.  No device needed. */
int flacmi_set_knob(const char* name, int32_t value);
int flacmi_get_knob(const char* name, int32_t* value);

/* ---- host-side views of the device arithmetic (for CPU verification of the helpers) ---- */
/* Python float `x ** 2` as CPython 3.10 + glibc 2.35 pow (FMA variant) computes it;
 * *status receives FLACMI_STATUS_OVERFLOW where Python raises OverflowError. */
double flacmi_host_pypow2(double x, int32_t* status);
/* floor(math.log2(x)) for finite x > 0, via the threshold table the device uses
 * (built once per process from libm log2); INT32_MIN for any other x. */
int32_t flacmi_host_floor_log2(double x);

/* The same helpers executed by the device kernels, over n host inputs (synchronous):
 * which = 0: out[i] = x[i] ** 2 (status[i] as flacmi_host_pypow2);
 * which = 1: out[i] = floor(log2(x[i])) for finite x[i] > 0. */
int flacmi_device_selftest(flacmi_ctx* ctx, int32_t which, const double* x, double* out,
                           int32_t* status, int64_t n);
/* k_lpc's Levinson-Durbin + quantiser (encoder.py:453-534) driven from n autocorrelation
 * rows acf[n][33] (lags 0..L used) instead of samples: rec[n][FLACMI_LPC_REC_WORDS(L)]
 * receives the LPC record k_lpc writes (word 0 = status | site << 16, word 1 = negative-shift
 * mask, then L shifts and the triangular coefficient table).  Reaches the overflow sites
 * (FLACMI_SITE_LEVINSON_POW, FLACMI_SITE_QUANT_LOG2) that no integer PCM block reaches
 * (DESIGN §4).  Synchronous; L in 1..32, q in 5..15. */
int flacmi_device_lpc_from_acf(flacmi_ctx* ctx, const double* acf, int64_t n, int32_t L, int32_t q,
                               int32_t* rec);

#ifdef __cplusplus
}
#endif
#endif /* FLACMI_H */
