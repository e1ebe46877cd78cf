/*
 * flacmi_host.cpp — the C-ABI of libflacmi.so (include/flacmi.h): contexts, argument
 * validation, per-length launch planning, tables computed from the host libm, and
 * device-memory helpers.  All compute is in the HIP kernels (k_*.hip).
 *
 * Host-side tables (built with the same libm CPython uses, so the device sees exactly
 * the values the reference computes):
 *   - Tukey(0.5) window per block length (flac/encoder.py:423-440, libm cos);
 *   - floor(log2(x)) thresholds per binary exponent (libm log2), for
 *     quantize_lpc_coefficients (encoder.py:503) and find_rice_parameter (:753);
 *   - the int16 sine table of the synthetic generator (libm sin).
 * This file is compiled with -ffp-contract=off like the kernels.
 */
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/flacmi.h"
#include "flacmi_kernels.h"
#include "pymath.h"
#include "device_common.h"

using namespace flacmi;

static double (*volatile libm_cos)(double) = cos;
static double (*volatile libm_log2)(double) = log2;
static double (*volatile libm_sin)(double) = sin;

/* ------------------------------------------------------------------------------------
 * errors
 * ---------------------------------------------------------------------------------- */
static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(FLACMI_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                            \
    } while (0)

/* ------------------------------------------------------------------------------------
 * process-wide host tables
 * ---------------------------------------------------------------------------------- */
static std::once_flag g_tables_once;
static std::vector<double> g_log2thr;   /* PYM_LOG2_THR_N */
static std::vector<int32_t> g_sintab;   /* 4096 */
static std::string g_tables_error;

static void build_tables() {
    g_log2thr.assign(PYM_LOG2_THR_N, 0.0);
    for (int e = -1074; e <= 1023; ++e) {
        const double hi = ldexp(1.0, e + 1); /* inf for e = 1023 */
        double thr = hi;
        {
            double x = nextafter(hi, 0.0); /* DBL_MAX for e = 1023 */
            while (x >= ldexp(1.0, e) && libm_log2(x) >= (double)(e + 1)) {
                thr = x;
                x = nextafter(x, 0.0);
            }
            /* monotonicity guard: nothing further below may reach e + 1 */
            for (int k = 0; k < 64 && x >= ldexp(1.0, e); ++k, x = nextafter(x, 0.0))
                if (libm_log2(x) >= (double)(e + 1)) g_tables_error = "libm log2 not monotonic near a power of two";
        }
        /* and nothing just above 2^e may fall below e */
        double y = ldexp(1.0, e);
        for (int k = 0; k < 64; ++k, y = nextafter(y, INFINITY))
            if (libm_log2(y) < (double)e) g_tables_error = "libm log2 below the exponent just above 2^e";
        g_log2thr[e + 1074] = thr;
    }
    g_sintab.resize(4096);
    for (int k = 0; k < 4096; ++k)
        g_sintab[k] = (int32_t)nearbyint(32767.0 * libm_sin(6.283185307179586 * (double)k / 4096.0));
}

static void ensure_tables() { std::call_once(g_tables_once, build_tables); }

/* CRC-16 tables of the frame writer (poly x^16 + x^15 + x^2 + 1, MSB first, init 0;
 * crc.py:25-31): [4][256] slice-by-4 tables T_k[v] = v * x^(16+8k) mod P, then for
 * b = 0..27 the linear map c -> c * x^(8*2^b) mod P as two 256-entry tables (low byte,
 * high byte of c), built by repeated squaring of the map. */
static std::vector<uint16_t> crc16_tables() {
    std::vector<uint16_t> t(4 * 256 + 28 * 512);
    auto mul8 = [&](uint32_t r) -> uint32_t { return ((r << 8) & 0xFFFF) ^ t[r >> 8]; };
    for (uint32_t v = 0; v < 256; ++v) {
        uint32_t r = v << 8;
        for (int i = 0; i < 8; ++i) r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1) & 0xFFFF;
        t[v] = (uint16_t)r;
    }
    for (int k = 1; k < 4; ++k)
        for (uint32_t v = 0; v < 256; ++v) t[k * 256 + v] = (uint16_t)mul8(t[(k - 1) * 256 + v]);
    uint32_t M[16], M2[16];
    for (int i = 0; i < 16; ++i) M[i] = mul8(1u << i);
    auto apply = [](const uint32_t* m, uint32_t c) {
        uint32_t r = 0;
        for (int i = 0; i < 16; ++i)
            if (c >> i & 1) r ^= m[i];
        return r;
    };
    for (int b = 0; b < 28; ++b) {
        uint16_t* o = t.data() + 4 * 256 + b * 512;
        for (uint32_t v = 0; v < 256; ++v) {
            o[v] = (uint16_t)apply(M, v);
            o[256 + v] = (uint16_t)apply(M, v << 8);
        }
        for (int i = 0; i < 16; ++i) M2[i] = apply(M, apply(M, 1u << i));
        memcpy(M, M2, sizeof M);
    }
    return t;
}

/* Tukey(0.5) window exactly as encoder.py:423-440 computes it; padded with zeros. */
static std::vector<double> tukey_window(int n, int pad) {
    std::vector<double> w((size_t)n + pad, 0.0);
    for (int i = 0; i < n; ++i) w[i] = 1.0;
    const int nr = (int)floor(0.25 * (double)n) - 1;
    if (nr > 0) {
        for (int i = 0; i < nr + 1; ++i) {
            w[i] = 0.5 - 0.5 * libm_cos(3.141592653589793 * (double)i / (double)nr);
            w[n - nr - 1 + i] = 0.5 - 0.5 * libm_cos(3.141592653589793 * (double)(i + nr) / (double)nr);
        }
    }
    return w;
}

/* ------------------------------------------------------------------------------------
 * context
 * ---------------------------------------------------------------------------------- */
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct flacmi_ctx {
    int device = 0;
    hipStream_t stream = nullptr; /* used by the host entry points */
    double* d_log2thr = nullptr;
    int32_t* d_sintab = nullptr;
    std::map<int, double*> windows;
    std::map<int, std::pair<int, int>> window_one; /* per n: [lo, hi) where the weight is 1.0 */
    std::map<int, uint16_t*> chunk_weights;        /* per n: the energy bound's weight per 8-sample chunk */
    DevBuf bound;                                  /* k_lpc's bound words [units][kBoundWords] */
    DevBuf rec, retry, h_samples, h_meta, h_params, h_residual, h_acf, h_fs, h_ls, h_recs;
    uint16_t* d_crc = nullptr;  /* CRC-16 slice tables [4][256] + power tables [28][512] */
    DevBuf scan, h_offsets, h_status, h_frames, dec, slow;
    DevBuf h_subkind;           /* flacmi_encode_host's sub_kind array (FLACMI_FRAME_FALLBACK) */
    DevBuf h_wasted;            /* flacmi_encode_host's wasted array (FLACMI_FRAME_WASTED) */
    DevBuf h_side, h_choice;    /* flacmi_encode_host's side rows and per-frame choice (FLACMI_STEREO_BEST) */
    DevBuf idx, sd_data, sd_table, sd_meta, sd_rows, sd_pcm; /* frame index workspace; flacmi_decode_stream_host's buffers */
    DevBuf si_frames, si_subs, si_parts; /* flacmi_info_stream_host's candidate records */
    /* flacmi_recompress_host: the frame list with its status words, the two carry buffers (int32 rows
     * of channels x rc_stride; rc_cur holds rc_carry_len samples a channel), the blocks written since
     * the last restart, and the last call's frame offsets / status for flacmi_recompress_fetch */
    DevBuf rc_list, rc_carry[2];
    int64_t rc_stride[2] = {0, 0};
    int rc_cur = 0, rc_channels = 0;
    int32_t rc_carry_len = 0;
    int64_t rc_blocks = 0;
    std::vector<int64_t> rc_offsets;
    std::vector<int32_t> rc_status;
    int64_t frames_bytes = 0;   /* bytes of the last flacmi_encode_host call */
    static constexpr int kRing = 64;
    static constexpr int kMaxChunks = 8;
    /* per call: start, LPC done, residual done, then (overlap) per chunk the k_resid start/end */
    hipEvent_t ev[kRing][3 + 2 * kMaxChunks] = {};
    int nchunks[kRing] = {};
    hipEvent_t lpc_done[kMaxChunks] = {}; /* k_lpc of chunk i finished (no timing) */
    int ncalls = 0; /* calls since the last timing reset */
    struct EncState* enc = nullptr; /* flacmi_encode_pipeline's streams, slots and pinned arrays */
    struct BatchState* batch = nullptr; /* flacmi_decode_batch_host's kept frame list */
};
static void enc_free(struct EncState* es);
static void batch_free(struct BatchState* bs);
static int enc_streams(flacmi_ctx* ctx);
static hipStream_t enc_side(flacmi_ctx* ctx);

static int ensure_buf(DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return 0;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    size_t want = bytes + bytes / 8 + 4096;
    HIP_TRY(hipMalloc(&b.p, want));
    b.bytes = want;
    return 0;
}

/* device row pitch in samples (flacmi_unit_stride) */
static int64_t row_pitch(int64_t n, int64_t sample_bytes) {
    int64_t bytes = ((n * sample_bytes + 15) / 16) * 16;
    if (bytes % 4096 == 0) bytes += 128;
    return bytes / sample_bytes;
}

static int set_device(flacmi_ctx* ctx) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    return 0;
}

/* flacmi_set_knob: environment read once, then atomics (no getenv on launch paths) */
namespace {
struct KnobDef {
    const char* name;
    int dflt;
};
constexpr KnobDef kKnobs[kKnobCount] = {{"FLACMI_OVERLAP", -1}, {"FLACMI_MF8_GRID", 0}, {"FLACMI_STREAM_GENERIC", 0}, {"FLACMI_DECODE_GENERIC", 0},
                                        {"FLACMI_PACK_GENERIC", 0}, {"FLACMI_DECODE_LPC", 1}, {"FLACMI_ENERGY_BOUND", 1}, {"FLACMI_INFO_GRID", 0},
                                        {"FLACMI_RICE_GRID", 0}};
std::atomic<int> g_knob[kKnobCount];
std::once_flag g_knob_once;
void knobs_init() {
    std::call_once(g_knob_once, [] {
        for (int i = 0; i < kKnobCount; ++i) {
            const char* e = getenv(kKnobs[i].name);
            g_knob[i].store(e && e[0] ? atoi(e) : kKnobs[i].dflt);
        }
    });
}
int knob_index(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < kKnobCount; ++i)
        if (strcmp(name, kKnobs[i].name) == 0) return i;
    return -1;
}
}  // namespace

int flacmi::knob(Knob k) {
    knobs_init();
    return g_knob[k].load(std::memory_order_relaxed);
}

extern "C" {

int flacmi_set_knob(const char* name, int32_t value) {
    const int i = knob_index(name);
    if (i < 0) return fail(FLACMI_E_INVALID, "unknown knob %s", name ? name : "(null)");
    knobs_init();
    g_knob[i].store(value);
    return 0;
}

int flacmi_get_knob(const char* name, int32_t* value) {
    const int i = knob_index(name);
    if (i < 0 || !value) return fail(FLACMI_E_INVALID, "unknown knob %s", name ? name : "(null)");
    *value = knob((Knob)i);
    return 0;
}

int flacmi_abi_version(void) { return FLACMI_ABI_VERSION; }

const char* flacmi_last_error(void) { return g_err.c_str(); }

int flacmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

flacmi_ctx* flacmi_create(int device) {
    ensure_tables();
    if (!g_tables_error.empty()) {
        fail(FLACMI_E_UNSUPPORTED, "%s", g_tables_error.c_str());
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fail(FLACMI_E_HIP, "no HIP device available");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail(FLACMI_E_INVALID, "device %d out of range (0..%d)", device, ndev - 1);
        return nullptr;
    }
    flacmi_ctx* ctx = new flacmi_ctx();
    ctx->device = device;
    auto bad = [&](hipError_t e, const char* what) {
        fail(FLACMI_E_HIP, "%s: %s", what, hipGetErrorString(e));
        flacmi_destroy(ctx);
        return (flacmi_ctx*)nullptr;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bad(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return bad(e, "hipStreamCreate");
    for (auto& slot : ctx->ev)
        for (auto& ev : slot)
            if ((e = hipEventCreate(&ev)) != hipSuccess) return bad(e, "hipEventCreate");
    for (auto& ev : ctx->lpc_done)
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    if ((e = hipMalloc(&ctx->d_log2thr, sizeof(double) * PYM_LOG2_THR_N)) != hipSuccess) return bad(e, "hipMalloc");
    if ((e = hipMemcpy(ctx->d_log2thr, g_log2thr.data(), sizeof(double) * PYM_LOG2_THR_N, hipMemcpyHostToDevice)) != hipSuccess)
        return bad(e, "hipMemcpy");
    if ((e = hipMalloc(&ctx->d_sintab, sizeof(int32_t) * 4096)) != hipSuccess) return bad(e, "hipMalloc");
    if ((e = hipMemcpy(ctx->d_sintab, g_sintab.data(), sizeof(int32_t) * 4096, hipMemcpyHostToDevice)) != hipSuccess)
        return bad(e, "hipMemcpy");
    const std::vector<uint16_t> crc = crc16_tables();
    if ((e = hipMalloc(&ctx->d_crc, sizeof(uint16_t) * crc.size())) != hipSuccess) return bad(e, "hipMalloc");
    if ((e = hipMemcpy(ctx->d_crc, crc.data(), sizeof(uint16_t) * crc.size(), hipMemcpyHostToDevice)) != hipSuccess)
        return bad(e, "hipMemcpy");
    return ctx;
}

void flacmi_destroy(flacmi_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    enc_free(ctx->enc);
    batch_free(ctx->batch);
    for (auto& kv : ctx->windows) (void)hipFree(kv.second);
    for (auto& kv : ctx->chunk_weights) (void)hipFree(kv.second);
    for (DevBuf* b : {&ctx->bound, &ctx->idx, &ctx->sd_data, &ctx->sd_table, &ctx->sd_meta, &ctx->sd_rows, &ctx->sd_pcm, &ctx->si_frames, &ctx->si_subs, &ctx->si_parts, &ctx->slow, &ctx->dec, &ctx->rec, &ctx->retry, &ctx->h_samples, &ctx->h_meta, &ctx->h_params, &ctx->h_residual, &ctx->h_acf,
                      &ctx->h_fs, &ctx->h_ls, &ctx->h_recs, &ctx->scan, &ctx->h_offsets, &ctx->h_status,
                      &ctx->h_frames, &ctx->h_subkind, &ctx->h_side, &ctx->h_choice, &ctx->h_wasted, &ctx->rc_list,
                      &ctx->rc_carry[0], &ctx->rc_carry[1]})
        if (b->p) (void)hipFree(b->p);
    if (ctx->d_log2thr) (void)hipFree(ctx->d_log2thr);
    if (ctx->d_sintab) (void)hipFree(ctx->d_sintab);
    if (ctx->d_crc) (void)hipFree(ctx->d_crc);
    for (auto& slot : ctx->ev)
        for (auto& ev : slot)
            if (ev) (void)hipEventDestroy(ev);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (auto& ev : ctx->lpc_done)
        if (ev) (void)hipEventDestroy(ev);
    delete ctx;
}

}  // extern "C"

/* The energy bound's two tables from the window's own weights.
 * kappa_k = max |w_i - w_{i-k}| over k <= i <= n - 2, rounded up, for k = 1 .. kBoundLags.
 * One weight per 8-sample chunk: floor(256 min w) over the chunk's samples, where sample
 * n - 1 (it never enters the autocorrelation) and the samples below 16 (at most 12 of them
 * are warm-up samples, which no candidate's sum holds) count as weight 0. */
static void bound_tables(const std::vector<double>& w, int n, double* kappa, std::vector<uint16_t>& cw) {
    for (int k = 1; k <= kBoundLags; ++k) {
        double m = 0.0;
        for (int i = k; i <= n - 2; ++i) m = std::max(m, fabs(w[i] - w[i - k]));
        kappa[k - 1] = m * (1.0 + ldexp(1.0, -50));
    }
    cw.assign((size_t)(n + 7) / 8, 0);
    for (int c = 2; 8 * c < n; ++c) {
        double m = 1.0;
        for (int i = 8 * c; i < 8 * c + 8; ++i) m = std::min(m, i < n - 1 ? w[i] : 0.0);
        cw[c] = (uint16_t)floor(256.0 * m);
    }
}

static int get_window(flacmi_ctx* ctx, int n, double** out, int* one_lo = nullptr, int* one_hi = nullptr,
                      const uint16_t** chunk_weight = nullptr) {
    auto it = ctx->windows.find(n);
    if (it == ctx->windows.end()) {
        std::vector<double> w = tukey_window(n, kWindowPad);
        std::vector<uint16_t> cw;
        w.resize(w.size() + kBoundLags, 0.0); /* kappa_1 .. behind the zero pad */
        bound_tables(w, n, w.data() + n + kWindowPad, cw);
        uint16_t* dcw = nullptr;
        HIP_TRY(hipMalloc(&dcw, sizeof(uint16_t) * cw.size()));
        HIP_TRY(hipMemcpy(dcw, cw.data(), sizeof(uint16_t) * cw.size(), hipMemcpyHostToDevice));
        ctx->chunk_weights[n] = dcw;
        double* d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(double) * w.size()));
        HIP_TRY(hipMemcpy(d, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
        ctx->windows[n] = d;
        /* the longest run of weights exactly 1.0 (the rectangle of encoder.py:433) */
        int best_lo = 0, best_hi = 0;
        for (int i = 0; i < n;) {
            if (w[i] != 1.0) {
                ++i;
                continue;
            }
            int j = i;
            while (j < n && w[j] == 1.0) ++j;
            if (j - i > best_hi - best_lo) {
                best_lo = i;
                best_hi = j;
            }
            i = j;
        }
        ctx->window_one[n] = {best_lo, best_hi};
        it = ctx->windows.find(n);
    }
    *out = it->second;
    if (one_lo) *one_lo = ctx->window_one[n].first;
    if (one_hi) *one_hi = ctx->window_one[n].second;
    if (chunk_weight) *chunk_weight = ctx->chunk_weights[n];
    return 0;
}

/* Largest candidate partition order for a block of n samples (predictor order 0). */
static int rice_max_eff(int n, int rmin, int rmax) {
    int r = -1;
    for (int o = rmin; o <= rmax; ++o)
        if (n % (1 << o) == 0) r = o;
    return r;
}

static int validate(const flacmi_batch* b, const flacmi_params* p, const flacmi_outputs* o) {
    if (!b || !p || !o) return fail(FLACMI_E_INVALID, "null argument");
    if (b->sample_bytes != 2 && b->sample_bytes != 4) return fail(FLACMI_E_INVALID, "sample_bytes must be 2 or 4");
    if (b->sample_bits < 2 || b->sample_bits > 8 * b->sample_bytes)
        return fail(FLACMI_E_INVALID, "sample_bits %d invalid for %d-byte samples", b->sample_bits, b->sample_bytes);
    if (b->n_units < 0 || b->n_tail_units < 0 || b->n_tail_units > b->n_units)
        return fail(FLACMI_E_INVALID, "bad unit counts");
    if (b->block_len < 1 || b->block_len > FLACMI_MAX_BLOCK) return fail(FLACMI_E_INVALID, "block_len out of range");
    if (b->n_tail_units > 0 && (b->tail_len < 1 || b->tail_len > b->block_len))
        return fail(FLACMI_E_INVALID, "tail_len out of range");
    if (b->unit_stride < b->block_len) return fail(FLACMI_E_INVALID, "unit_stride < block_len");
    if ((b->unit_stride * b->sample_bytes) % 16 != 0 || ((uintptr_t)b->samples % 16) != 0)
        return fail(FLACMI_E_INVALID, "sample rows must be 16-byte aligned");
    if (p->max_lpc_order < 0 || p->max_lpc_order > FLACMI_MAX_LPC_ORDER)
        return fail(FLACMI_E_INVALID, "max_lpc_order must be 0..32");
    if (p->qlp_precision < 5 || p->qlp_precision > 31) return fail(FLACMI_E_INVALID, "qlp_precision must be 5..31");
    if (p->rice_min < 0 || p->rice_max > FLACMI_MAX_RICE_ORDER)
        return fail(FLACMI_E_INVALID, "rice partition orders must be within 0..15");
    if (p->mode < FLACMI_MODE_REFERENCE || p->mode > FLACMI_MODE_RICE_ONLY) return fail(FLACMI_E_INVALID, "bad mode");
    if (p->mode == FLACMI_MODE_RICE_ONLY && (p->reserved[0] < 0 || p->reserved[0] > FLACMI_MAX_LPC_ORDER))
        return fail(FLACMI_E_INVALID, "RICE_ONLY predictor order (reserved[0]) must be 0..32");
    if (p->mode == FLACMI_MODE_LPC_ONLY && p->max_lpc_order < 1)
        return fail(FLACMI_E_INVALID, "LPC_ONLY needs max_lpc_order >= 1");
    if ((p->reserved[1] & FLACMI_FLAG_LPC_SIGN) && (p->mode == FLACMI_MODE_FIXED_ONLY || p->mode == FLACMI_MODE_RICE_ONLY))
        return fail(FLACMI_E_INVALID, "FLACMI_FLAG_LPC_SIGN needs FLACMI_MODE_REFERENCE or FLACMI_MODE_LPC_ONLY");
    if ((p->reserved[1] & FLACMI_FLAG_RICE_SEARCH) && p->mode == FLACMI_MODE_LPC_ONLY)
        return fail(FLACMI_E_INVALID, "FLACMI_FLAG_RICE_SEARCH: FLACMI_MODE_LPC_ONLY has no Rice step");
    if ((p->reserved[1] & FLACMI_FLAG_RICE_SEARCH) && p->rice_max > 8)
        return fail(FLACMI_E_INVALID, "FLACMI_FLAG_RICE_SEARCH needs rice_max <= 8 (the FLAC subset bound)");
    if (p->reserved[1] & FLACMI_FLAG_SIZE_CHOICE) {
        if (!(p->reserved[1] & FLACMI_FLAG_RICE_SEARCH))
            return fail(FLACMI_E_INVALID, "FLACMI_FLAG_SIZE_CHOICE needs FLACMI_FLAG_RICE_SEARCH (sizes are the exact search's)");
        if (p->mode != FLACMI_MODE_REFERENCE && p->mode != FLACMI_MODE_FIXED_ONLY)
            return fail(FLACMI_E_INVALID, "FLACMI_FLAG_SIZE_CHOICE needs FLACMI_MODE_REFERENCE or FLACMI_MODE_FIXED_ONLY");
        if (p->reserved[2] < 0 || p->reserved[2] > 33)
            return fail(FLACMI_E_INVALID, "FLACMI_FLAG_SIZE_CHOICE: the written sample width (reserved[2]) must be 0..33");
        const int L = p->mode == FLACMI_MODE_REFERENCE ? p->max_lpc_order : 0;
        const size_t lds = size_choice_lds(b->block_len, b->sample_bytes, FLACMI_LPC_REC_WORDS(L), p->rice_max);
        if (lds > 160 * 1024)
            return fail(FLACMI_E_UNSUPPORTED, "block of %d samples needs %zu bytes of LDS", b->block_len, lds);
    }
    if (p->mode != FLACMI_MODE_FIXED_ONLY && p->mode != FLACMI_MODE_RICE_ONLY && b->sample_bits + p->qlp_precision > 44)
        return fail(FLACMI_E_UNSUPPORTED,
                    "sample_bits + qlp_precision > 44: candidate residual sums may exceed int64 (see DESIGN.md)");
    if (o->residual_bytes != 4 && o->residual_bytes != 8) return fail(FLACMI_E_INVALID, "residual_bytes must be 4 or 8");
    if (o->residual_stride < b->block_len || (o->residual_stride * o->residual_bytes) % 16 != 0 ||
        ((uintptr_t)o->residual % 16) != 0)
        return fail(FLACMI_E_INVALID, "residual rows must hold block_len elements and be 16-byte aligned");
    if (!o->meta || !o->rice_params || !o->residual) return fail(FLACMI_E_INVALID, "null output buffer");
    const int lens[2] = {b->block_len, b->n_tail_units ? b->tail_len : b->block_len};
    for (int n : lens) {
        const int re = rice_max_eff(n, p->rice_min, p->rice_max);
        if (re >= 0 && (1 << re) > kMaxFinestParts)
            return fail(FLACMI_E_UNSUPPORTED, "2^%d Rice partitions exceed the %d this build stages in LDS", re,
                        kMaxFinestParts);
        if (re >= 0 && o->params_stride < (1 << re)) return fail(FLACMI_E_INVALID, "params_stride < 2^%d", re);
        const ResidLaunch rl = resid_launch_config(n, re, o->residual_bytes);
        if (rl.lds_bytes > 160 * 1024)
            return fail(FLACMI_E_UNSUPPORTED, "block of %d samples needs %zu bytes of LDS", n, rl.lds_bytes);
    }
    return 0;
}

/* int32 arithmetic is exact when every |prediction| and |residual| < 2^26 and a thread's
 * partial sum of |r| over the samples it owns still fits 32 bits.  Otherwise int64. */
static bool needs_wide(int n, int bits, int L, int q, int mode) {
    if (bits > 24 || q > 24) return true;
    const double xmax = ldexp(1.0, bits - 1);
    const double rmax = (mode == FLACMI_MODE_FIXED_ONLY || mode == FLACMI_MODE_RICE_ONLY) ? 16.0 * xmax : xmax * (1.0 + (double)L * ldexp(1.0, q - 1)) + 16.0 * xmax;
    return rmax >= ldexp(1.0, 26) || rmax * resid_samples_per_thread(n) >= ldexp(1.0, 32);
}

/* PATH_W64S preconditions: samples <= 24 bits and q <= 16 (every sample plane, coefficient
 * and -2^shift fits int16), and each plane's dot chain stays inside int32:
 * max|plane| * (L * 2^(q-1) + 2^15) < 2^31.  Opt-in (FLACMI_SPLIT=1): on MI355X it
 * measured slower than PATH_W64's v_mad_i64_i32 chains (c3: 71.0 vs 67.1 ms), the plane
 * build costing more than the dot2 pairing saves. */
static bool split_ok(int bits, int L, int q) {
    static const int off = [] {
        const char* e = getenv("FLACMI_SPLIT");
        return (e && atoi(e) != 0) ? 0 : 1;
    }();
    if (off || bits > 24 || q > 16 || L < 1) return false;
    const double plane = bits > 24 - 12 ? ldexp(1.0, bits - 13) : 0.0;
    const double pmax = plane > 2048.0 ? plane : 2048.0;
    return pmax * ((double)L * ldexp(1.0, q - 1) + 32768.0) < ldexp(1.0, 31);
}

/* FLACMI_DEBUG_STOP=k truncates k_resid after phase k (profiling ablation only: the
 * outputs are then incomplete). */
static int debug_stop() {
    static const int v = [] {
        const char* e = getenv("FLACMI_DEBUG_STOP");
        return e ? atoi(e) : 0;
    }();
    return v;
}

/* FLACMI_NO_MFMA=1 keeps the candidate sums on the VALU path (comparison runs). */
static int use_mfma() {
    static const int v = [] {
        const char* e = getenv("FLACMI_NO_MFMA");
        return (e && atoi(e) != 0) ? 0 : 1;
    }();
    return v;
}

/* FLACMI_NO_STREAM=1 keeps k_resid's one-workgroup-per-unit kernels (comparison runs). */
static int use_stream() {
    static const int v = [] {
        const char* e = getenv("FLACMI_NO_STREAM");
        return (e && atoi(e) != 0) ? 0 : 1;
    }();
    return v;
}

/* FLACMI_NO_SIGNBOUND=1 prunes the int8-MFMA path with the partial-sum tiers alone, as
 * FLACMI_FLAG_TIERS_ONLY does per call (A/B runs). */
static int sign_bound_allowed() {
    static const int v = [] {
        const char* e = getenv("FLACMI_NO_SIGNBOUND");
        return (e && atoi(e) != 0) ? 0 : 1;
    }();
    return v;
}

/* FLACMI_NO_PRUNE=1 computes every LPC candidate's exact sum in reference mode, as
 * FLACMI_FLAG_ALL_CANDIDATES does per call (comparison runs). */
static int prune_allowed() {
    static const int v = [] {
        const char* e = getenv("FLACMI_NO_PRUNE");
        return (e && atoi(e) != 0) ? 0 : 1;
    }();
    return v;
}

/* k_lpc and k_resid of consecutive chunks overlap on two streams (see analyze_device_impl).
 * FLACMI_OVERLAP (flacmi_set_knob; the environment's value at first use): unset or -1 = round-aligned (the default): the units of
 * k_lpc's whole rounds, then the remainder (a partly filled last round), whose k_lpc runs
 * beside k_resid of the first chunk, when the remainder holds at least kOverlapMinUnits;
 * 0 = no overlap; k > 1 = up to k equal chunks of at least kOverlapMinUnits; -R (R > 1) =
 * round-aligned with R units per round and no minimum (tests). */
constexpr int64_t kOverlapMinUnits = 16384;
#ifndef FLACMI_CLASS_LISTS
#define FLACMI_CLASS_LISTS 1 /* A/B build (timing only, same results): 0 runs every chunk's list passes behind its batch kernel */
#endif
static int overlap_mode() { return knob(kKnobOverlap); }

static int analyze_device_impl(flacmi_ctx* ctx, const flacmi_batch* b, const flacmi_params* p,
                               const flacmi_outputs* o, hipStream_t s, bool allow_overlap = true) {
    if (int rc = set_device(ctx)) return rc;
    const bool lpc = p->mode == FLACMI_MODE_REFERENCE || p->mode == FLACMI_MODE_LPC_ONLY;
    const int L = lpc ? p->max_lpc_order : 0;
    const int rec_words = FLACMI_LPC_REC_WORDS(L);
    if (lpc) {
        if (int rc = ensure_buf(ctx->rec, sizeof(int32_t) * (size_t)rec_words * (size_t)(b->n_units > 0 ? b->n_units : 1)))
            return rc;
    }
    /* the energy bound (k_lpc's words, k_resid_stream's pre-test): wherever the stream kernel may prune */
    const int energy = debug_stop() >= 11 ? 0 : knob(kKnobEnergyBound); /* (the tier ablations time the tiers) */
    const bool prune_call = p->mode == FLACMI_MODE_REFERENCE && !o->lpc_sums &&
                            !(p->reserved[1] & (FLACMI_FLAG_ALL_CANDIDATES | FLACMI_FLAG_LPC_SIGN | FLACMI_FLAG_SIZE_CHOICE)) && prune_allowed();
    const bool ebound = energy != 0 && prune_call && L >= 1 && L <= 12 && b->sample_bytes == 2 && p->qlp_precision <= 16;
    if (ebound) {
        if (int rc = ensure_buf(ctx->bound, sizeof(uint32_t) * kBoundWords * (size_t)(b->n_units > 0 ? b->n_units : 1))) return rc;
    }
    /* fast-kernel retry lists: 64 sub-list counters (k_resid_stream's batch kernel, 128 B apart),
     * a counter and one batch index per unit (plus 64 for the sub-lists' rounding), then the
     * second list through which k_resid_stream's list kernel hands units on */
    constexpr int64_t kSubWords = 64 * 16;
    if (int rc = ensure_buf(ctx->retry, sizeof(int64_t) * (size_t)(kSubWords + 2 * b->n_units + 68))) return rc;
    struct Cls {
        int64_t unit0, count;
        int n;
    } cls[2];
    int ncls = 0;
    const int64_t nfull = b->n_units - b->n_tail_units;
    if (b->n_tail_units == 0 || b->tail_len == b->block_len) {
        cls[ncls++] = {0, b->n_units, b->block_len};
    } else {
        if (nfull > 0) cls[ncls++] = {0, nfull, b->block_len};
        cls[ncls++] = {nfull, b->n_tail_units, b->tail_len};
    }
    if (o->acf && !lpc)
        HIP_TRY(hipMemsetAsync(o->acf, 0, sizeof(double) * 33 * b->n_units, s));
    /* Units in chunks of one class each.  Without overlap: one chunk per class, the LPC
     * pass over all of them, then the residual pass, in order on s.  With overlap
     * (FLACMI_OVERLAP=k > 1): each class in up to k chunks; k_lpc runs the chunks in order
     * on the side stream and k_resid of chunk i (on s) waits only for k_lpc of chunk i, so
     * the f64 autocorrelation of chunk i+1 shares the GPU with the integer/MFMA work of
     * chunk i. */
    struct Chunk {
        int64_t unit0, count;
        int n;
    } ch[flacmi_ctx::kMaxChunks];
    auto lpc_params_for = [&](int n) {
        LpcArgs a{};
        a.stride = b->unit_stride;
        a.sample_bytes = b->sample_bytes;
        a.n = n;
        a.L = L;
        return a;
    };
    int nch = 0;
    const int ov = lpc ? overlap_mode() : 0;
    const int want = ov > 1 ? ov : 1;
    bool overlap = want > 1 && b->n_units >= 2 * kOverlapMinUnits;
    for (int c = 0; c < ncls; ++c) {
        if (ov < -1 || (ov == -1 && cls[c].count >= 2 * kOverlapMinUnits)) {
            /* round-aligned: the units of k_lpc's whole rounds, then the remainder, whose
             * k_lpc fills the last round's idle slots beside k_resid of the first chunk */
            const int64_t R = ov < -1 ? -(int64_t)ov : lpc_units_per_round(lpc_params_for(cls[c].n));
            const int64_t whole = R > 0 ? cls[c].count / R * R : 0, rest = cls[c].count - whole;
            if (whole > 0 && rest > 0 && (ov < -1 || rest >= kOverlapMinUnits) &&
                nch + 2 + (ncls - 1 - c) <= flacmi_ctx::kMaxChunks) {
                ch[nch++] = {cls[c].unit0, whole, cls[c].n};
                ch[nch++] = {cls[c].unit0 + whole, rest, cls[c].n};
                overlap = true;
                continue;
            }
        }
        int64_t k = overlap && ov > 1 ? cls[c].count / kOverlapMinUnits : 1;
        const int left = flacmi_ctx::kMaxChunks - nch - (ncls - 1 - c);
        k = k < 1 ? 1 : k > want ? want : k;
        k = k > left ? left : k;
        for (int64_t i = 0; i < k; ++i) {
            const int64_t u0 = cls[c].count * i / k, u1 = cls[c].count * (i + 1) / k;
            ch[nch++] = {cls[c].unit0 + u0, u1 - u0, cls[c].n};
        }
    }
    auto lpc_args = [&](const Chunk& k, LpcArgs& a) -> int {
        a = LpcArgs{};
        a.samples = b->samples;
        a.stride = b->unit_stride;
        a.unit0 = k.unit0;
        a.count = k.count;
        a.sample_bytes = b->sample_bytes;
        a.n = k.n;
        a.L = L;
        a.q = p->qlp_precision;
        a.lpc_sign = (p->reserved[1] & FLACMI_FLAG_LPC_SIGN) != 0;
        if (int rc = get_window(ctx, k.n, (double**)&a.window, &a.fuse_lo, &a.fuse_hi)) return rc;
        a.bound = ebound ? (uint32_t*)ctx->bound.p + kBoundWords * k.unit0 : nullptr;
        if (b->sample_bits > 26) a.fuse_lo = a.fuse_hi = 0; /* products must stay below 2^52 */
        a.log2thr = ctx->d_log2thr;
        a.rec = (int32_t*)ctx->rec.p + k.unit0 * rec_words;
        a.rec_words = rec_words;
        a.acf = o->acf ? o->acf + k.unit0 * 33 : nullptr;
        return 0;
    };
    /* the residual pass's arguments for units [k.unit0, k.unit0 + k.count) and the path it takes */
    auto resid_args = [&](const Chunk& k, ResidArgs& a, int& path) -> hipError_t {
        a = ResidArgs{};
        a.samples = b->samples;
        a.stride = b->unit_stride;
        a.unit0 = k.unit0;
        a.count = k.count;
        a.sample_bytes = b->sample_bytes;
        a.n = k.n;
        a.L = L;
        a.mode = p->mode;
        a.rmin = p->rice_min;
        a.rmax = p->rice_max;
        a.rec = lpc ? (const int32_t*)ctx->rec.p + k.unit0 * rec_words : nullptr;
        a.rice_order = p->mode == FLACMI_MODE_RICE_ONLY ? p->reserved[0] : 0;
        a.rec_words = rec_words;
        a.log2thr = ctx->d_log2thr;
        a.meta = o->meta + k.unit0;
        a.rice_params = o->rice_params + k.unit0 * o->params_stride;
        a.params_stride = o->params_stride;
        a.residual = (char*)o->residual + (size_t)k.unit0 * o->residual_stride * o->residual_bytes;
        a.residual_stride = o->residual_stride;
        a.fixed_sums = o->fixed_sums ? o->fixed_sums + k.unit0 * 5 : nullptr;
        a.lpc_sums = o->lpc_sums ? o->lpc_sums + k.unit0 * 32 : nullptr;
        a.stop_after = debug_stop();
        a.mfma = use_mfma();
        int64_t* const rb = (int64_t*)ctx->retry.p;
        a.retry_sub = (unsigned long long*)rb;
        a.retry_count = (unsigned long long*)(rb + kSubWords);
        a.retry_list = rb + kSubWords + 2;
        a.retry2_count = (unsigned long long*)(rb + kSubWords + 2 + b->n_units + 64);
        a.retry2_list = rb + kSubWords + 4 + b->n_units + 64;
        a.sample_bits = b->sample_bits;
        a.stream = use_stream();
        /* every bound the kernels hold proves "LPC loses", the rare case once the predictor has
         * its sign: FLACMI_FLAG_LPC_SIGN computes every candidate's exact sum */
        a.prune = prune_call;
        if (ebound) {
            double* w = nullptr;
            if (get_window(ctx, k.n, &w, nullptr, nullptr, &a.chunk_weight)) return hipErrorOutOfMemory;
            a.bound = (const uint32_t*)ctx->bound.p + kBoundWords * k.unit0;
            a.energy = energy;
        }
        a.sign_bound = !(p->reserved[1] & FLACMI_FLAG_TIERS_ONLY) && sign_bound_allowed();
        const bool wide = needs_wide(k.n, b->sample_bits, L, p->qlp_precision, p->mode);
        path = (wide || o->residual_bytes == 8) ? 2 : (b->sample_bytes == 2 && p->qlp_precision <= 16) ? 0 : 1;
        if (path == 2 && o->residual_bytes == 4 && split_ok(b->sample_bits, L, p->qlp_precision)) path = 3;
        return hipSuccess;
    };
    auto launch_resid_chunk = [&](const Chunk& k, hipStream_t st) -> hipError_t {
        ResidArgs a;
        int path = 0;
        if (hipError_t e = resid_args(k, a, path); e != hipSuccess) return e;
        return launch_resid(a, path, o->residual_bytes, st);
    };
    const int slot = ctx->ncalls % flacmi_ctx::kRing;
    hipEvent_t* ev = ctx->ev[slot];
    hipStream_t side = nullptr;
    if (overlap && !allow_overlap) overlap = false;
    if (overlap) {
        /* k_lpc runs on the pipeline's H2D stream, which lives as long as the context: a
         * stream created here would have to be destroyed before returning, and destroying a
         * stream with queued work waits for it (the call would block the host).  A stream
         * left open instead takes a hardware queue that the pipeline's copies then share
         * (measured: the 1e5-unit host-to-host encode 20.4 -> 38.5 ms wall). */
        if (int rc = enc_streams(ctx)) return rc;
        side = enc_side(ctx);
        if (side == s) overlap = false;
    }
    /* FLACMI_FLAG_SIZE_CHOICE: k_lpc, then k_size_choice alone writes every unit (no k_resid, no k_rice_search) */
    const bool size_choice = (p->reserved[1] & FLACMI_FLAG_SIZE_CHOICE) != 0;
    if (size_choice) overlap = false;
    ctx->nchunks[slot] = overlap ? nch : 0;
    HIP_TRY(hipEventRecord(ev[0], s));
    if (overlap) {
        HIP_TRY(hipStreamWaitEvent(side, ev[0], 0));
        for (int i = 0; i < nch; ++i) {
            LpcArgs a;
            if (int rc = lpc_args(ch[i], a)) return rc;
            HIP_TRY(launch_lpc(a, side));
            HIP_TRY(hipEventRecord(ctx->lpc_done[i], side));
        }
        HIP_TRY(hipEventRecord(ev[1], side));
        for (int i = 0; i < nch;) {
            /* the chunks [i, j) of one length class.  Where they take k_resid_stream's pre-test build,
             * their batch kernels run back to back (the counters zeroed once, ids listed relative to
             * the class) and one list pass and one retry pass follow the last: no list launch, retry
             * kernel or memset drains the GPU between two batch kernels.  Each chunk's timing span
             * holds its batch kernel, the first's the memsets too, the last's both list passes. */
            int j = i + 1;
            while (j < nch && ch[j].n == ch[i].n && ch[j].unit0 == ch[j - 1].unit0 + ch[j - 1].count) ++j;
            ResidArgs ca;
            int cpath = 0;
            const Chunk whole{ch[i].unit0, ch[j - 1].unit0 + ch[j - 1].count - ch[i].unit0, ch[i].n};
            HIP_TRY(resid_args(whole, ca, cpath));
            const bool merged = FLACMI_CLASS_LISTS && j - i > 1 && stream_class_ok(ca, cpath, o->residual_bytes);
            for (int c = i; c < j; ++c) {
                HIP_TRY(hipStreamWaitEvent(s, ctx->lpc_done[c], 0));
                HIP_TRY(hipEventRecord(ev[3 + 2 * c], s));
                if (merged) {
                    ResidArgs a;
                    int path = 0;
                    HIP_TRY(resid_args(ch[c], a, path));
                    if (c == i) HIP_TRY(launch_stream_class_begin(ca, s));
                    HIP_TRY(launch_stream_class_batch(a, ch[c].unit0 - whole.unit0, whole.count, s));
                    if (c == j - 1) HIP_TRY(launch_stream_class_lists(ca, s));
                } else {
                    HIP_TRY(launch_resid_chunk(ch[c], s));
                }
                HIP_TRY(hipEventRecord(ev[4 + 2 * c], s));
            }
            i = j;
        }
    } else {
        for (int i = 0; i < nch && lpc; ++i) {
            LpcArgs a;
            if (int rc = lpc_args(ch[i], a)) return rc;
            HIP_TRY(launch_lpc(a, s));
        }
        HIP_TRY(hipEventRecord(ev[1], s));
        for (int i = 0; i < nch && !size_choice; ++i) HIP_TRY(launch_resid_chunk(ch[i], s));
    }
    if (size_choice) {
        SizeArgs sa{};
        sa.samples = b->samples;
        sa.stride = b->unit_stride;
        sa.sample_bytes = b->sample_bytes;
        sa.block_len = b->block_len;
        sa.tail_len = b->n_tail_units ? b->tail_len : b->block_len;
        sa.n_units = b->n_units;
        sa.n_tail_units = b->n_tail_units;
        sa.L = L;
        sa.q = p->qlp_precision;
        sa.mode = p->mode;
        sa.rmin = p->rice_min;
        sa.rmax = p->rice_max;
        sa.ss = p->reserved[2] ? p->reserved[2] : b->sample_bits;
        sa.rec = lpc ? (const int32_t*)ctx->rec.p : nullptr;
        sa.rec_words = rec_words;
        sa.meta = o->meta;
        sa.rice_params = o->rice_params;
        sa.params_stride = o->params_stride;
        sa.residual = o->residual;
        sa.residual_stride = o->residual_stride;
        sa.fixed_sums = o->fixed_sums;
        sa.lpc_sums = o->lpc_sums;
        if (debug_stop() == 0) HIP_TRY(launch_size_choice(sa, o->residual_bytes, knob(kKnobRiceGrid), s));
    } else if (p->reserved[1] & FLACMI_FLAG_RICE_SEARCH) {
        /* behind the last k_resid launch (list and retry passes included): every unit has its final status */
        RiceArgs ra{};
        ra.meta = o->meta;
        ra.rice_params = o->rice_params;
        ra.params_stride = o->params_stride;
        ra.residual = o->residual;
        ra.residual_stride = o->residual_stride;
        ra.n_units = b->n_units;
        ra.n_tail_units = b->n_tail_units;
        ra.block_len = b->block_len;
        ra.tail_len = b->n_tail_units ? b->tail_len : b->block_len;
        ra.rmin = p->rice_min;
        ra.rmax = p->rice_max;
        ra.mode = p->mode;
        ra.rice_order = p->mode == FLACMI_MODE_RICE_ONLY ? p->reserved[0] : 0;
        if (debug_stop() == 0) HIP_TRY(launch_rice_search(ra, o->residual_bytes, knob(kKnobRiceGrid), s));
    }
    HIP_TRY(hipEventRecord(ev[2], s));
    ctx->ncalls++;
    if (o->lpc_records) {
        if (lpc) {
            HIP_TRY(launch_expand_records((const int32_t*)ctx->rec.p, rec_words, L, b->n_units, o->lpc_records, s));
        } else {
            HIP_TRY(hipMemsetAsync(o->lpc_records, 0, sizeof(int32_t) * FLACMI_LPC_REC_WORDS(32) * b->n_units, s));
        }
    }
    return 0;
}

extern "C" {

int flacmi_analyze_device(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_params* params,
                          const flacmi_outputs* out, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (int rc = validate(batch, params, out)) return rc;
    if (batch->n_units == 0) return 0;
    return analyze_device_impl(ctx, batch, params, out, (hipStream_t)stream);
}

int flacmi_analyze_host(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_params* params,
                        const flacmi_outputs* out) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (!batch || !params || !out) return fail(FLACMI_E_INVALID, "null argument");
    if (batch->n_units == 0) return 0;
    if (int rc = set_device(ctx)) return rc;
    const size_t nu = (size_t)batch->n_units;
    /* device mirrors with 16-byte aligned rows */
    const int64_t sstride = row_pitch(batch->block_len, batch->sample_bytes);
    const int64_t rstride = ((batch->block_len * out->residual_bytes + 15) / 16) * 16 / out->residual_bytes;
    if (int rc = ensure_buf(ctx->h_samples, nu * sstride * batch->sample_bytes)) return rc;
    if (int rc = ensure_buf(ctx->h_meta, nu * sizeof(flacmi_unit_meta))) return rc;
    if (int rc = ensure_buf(ctx->h_params, nu * out->params_stride * sizeof(int32_t))) return rc;
    if (int rc = ensure_buf(ctx->h_residual, nu * rstride * out->residual_bytes)) return rc;
    flacmi_batch db = *batch;
    db.samples = ctx->h_samples.p;
    db.unit_stride = sstride;
    HIP_TRY(hipMemcpy2DAsync(ctx->h_samples.p, sstride * batch->sample_bytes, batch->samples,
                             batch->unit_stride * batch->sample_bytes, batch->block_len * batch->sample_bytes, nu,
                             hipMemcpyHostToDevice, ctx->stream));
    flacmi_outputs dout = *out;
    dout.meta = (flacmi_unit_meta*)ctx->h_meta.p;
    dout.rice_params = (int32_t*)ctx->h_params.p;
    dout.residual = ctx->h_residual.p;
    dout.residual_stride = rstride;
    if (out->acf) {
        if (int rc = ensure_buf(ctx->h_acf, nu * 33 * sizeof(double))) return rc;
        dout.acf = (double*)ctx->h_acf.p;
    }
    if (out->fixed_sums) {
        if (int rc = ensure_buf(ctx->h_fs, nu * 5 * sizeof(int64_t))) return rc;
        dout.fixed_sums = (int64_t*)ctx->h_fs.p;
    }
    if (out->lpc_sums) {
        if (int rc = ensure_buf(ctx->h_ls, nu * 32 * sizeof(int64_t))) return rc;
        dout.lpc_sums = (int64_t*)ctx->h_ls.p;
    }
    if (out->lpc_records) {
        if (int rc = ensure_buf(ctx->h_recs, nu * FLACMI_LPC_REC_WORDS(32) * sizeof(int32_t))) return rc;
        dout.lpc_records = (int32_t*)ctx->h_recs.p;
    }
    if (int rc = validate(&db, params, &dout)) return rc;
    if (int rc = analyze_device_impl(ctx, &db, params, &dout, ctx->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(out->meta, dout.meta, nu * sizeof(flacmi_unit_meta), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out->rice_params, dout.rice_params, nu * out->params_stride * sizeof(int32_t),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(out->residual, out->residual_stride * out->residual_bytes, dout.residual,
                             rstride * out->residual_bytes, batch->block_len * out->residual_bytes, nu,
                             hipMemcpyDeviceToHost, ctx->stream));
    if (out->acf)
        HIP_TRY(hipMemcpyAsync(out->acf, dout.acf, nu * 33 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (out->fixed_sums)
        HIP_TRY(hipMemcpyAsync(out->fixed_sums, dout.fixed_sums, nu * 5 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out->lpc_sums)
        HIP_TRY(hipMemcpyAsync(out->lpc_sums, dout.lpc_sums, nu * 32 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out->lpc_records)
        HIP_TRY(hipMemcpyAsync(out->lpc_records, dout.lpc_records, nu * FLACMI_LPC_REC_WORDS(32) * sizeof(int32_t),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"

/* ---- frame writer ---------------------------------------------------------------- */
static int validate_frames(const flacmi_batch* b, const flacmi_frame_params* fp, int64_t* n_frames) {
    if (!b || !fp) return fail(FLACMI_E_INVALID, "null argument");
    if (fp->channels < 1 || fp->channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (fp->sample_size < 1 || fp->sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 1..32");
    if (fp->qlp_precision < 5 || fp->qlp_precision > 31) return fail(FLACMI_E_INVALID, "qlp_precision must be 5..31");
    if (fp->first_frame < 0) return fail(FLACMI_E_INVALID, "first_frame must be >= 0");
    if (fp->reserved0 & ~(FLACMI_FRAME_FALLBACK | FLACMI_FRAME_WASTED))
        return fail(FLACMI_E_INVALID, "unknown frame flag bits %#x (reserved0)", (unsigned)fp->reserved0);
    if ((fp->reserved0 & FLACMI_FRAME_WASTED) && fp->reserved[1] != FLACMI_STEREO_OFF)
        return fail(FLACMI_E_INVALID, "FLACMI_FRAME_WASTED does not combine with the stereo mode (reserved[1])");
    if (fp->reserved[1] != FLACMI_STEREO_OFF && fp->reserved[1] != FLACMI_STEREO_BEST)
        return fail(FLACMI_E_INVALID, "unknown stereo mode %lld (reserved[1])", (long long)fp->reserved[1]);
    if (fp->reserved[1] == FLACMI_STEREO_BEST && (fp->channels != 2 || fp->sample_size > 31))
        return fail(FLACMI_E_INVALID, "the stereo mode (reserved[1]) needs channels == 2 and sample_size <= 31");
    if (b->n_units % fp->channels != 0) return fail(FLACMI_E_INVALID, "n_units must be a multiple of channels");
    if (b->n_tail_units != 0 && b->n_tail_units != fp->channels)
        return fail(FLACMI_E_INVALID, "the short last frame must hold exactly `channels` tail units");
    if (b->block_len < 1 || b->block_len > FLACMI_MAX_BLOCK) return fail(FLACMI_E_INVALID, "block_len out of range");
    *n_frames = b->n_units / fp->channels;
    return 0;
}

static FrameArgs frame_args(flacmi_ctx* ctx, const flacmi_batch* b, const flacmi_frame_params* fp,
                            const flacmi_unit_meta* meta, const int32_t* rice_params, int64_t params_stride,
                            int64_t n_frames) {
    FrameArgs a{};
    a.samples = b->samples;
    a.stride = b->unit_stride;
    a.sample_bytes = b->sample_bytes;
    a.block_len = b->block_len;
    a.tail_len = b->n_tail_units ? b->tail_len : b->block_len;
    a.n_units = b->n_units;
    a.n_tail_units = b->n_tail_units;
    a.channels = fp->channels;
    a.sample_size = fp->sample_size;
    a.q = fp->qlp_precision;
    a.first_frame = fp->first_frame;
    a.n_frames = n_frames;
    a.meta = meta;
    a.rice_params = rice_params;
    a.params_stride = params_stride;
    a.crc_slice = ctx->d_crc;
    a.crc_pow = ctx->d_crc + 4 * 256;
    return a;
}

/* FLACMI_FRAME_FALLBACK at the *_device entry points: the caller's sub_kind array */
static int caller_sub_kind(const flacmi_frame_params* fp, FrameArgs& a) {
    if (!(fp->reserved0 & FLACMI_FRAME_FALLBACK)) return 0;
    a.sub_kind = (int32_t*)(uintptr_t)fp->reserved[0];
    if (!a.sub_kind) return fail(FLACMI_E_INVALID, "FLACMI_FRAME_FALLBACK needs a sub_kind array in reserved[0]");
    return 0;
}

/* the same for the host entry points: an array of their own (a context buffer, or one per
 * pipeline slot); in the stereo mode (a.choice set before this) over the 4 n_frames candidates */
static int own_sub_kind(const flacmi_frame_params* fp, DevBuf& buf, FrameArgs& a) {
    if (!(fp->reserved0 & FLACMI_FRAME_FALLBACK)) return 0;
    if (int rc = ensure_buf(buf, sizeof(int32_t) * (size_t)a.n_units * (a.choice ? 2 : 1))) return rc;
    a.sub_kind = (int32_t*)buf.p;
    return 0;
}

/* ---- stereo mode (FLACMI_STEREO_BEST) at the host entry points --------------------------
 * A sub-batch of nu = 2 F caller units has 4 F candidate units (frame_bits.h): the analysis
 * outputs hold 2 nu units, the sample buffer nu + F rows (the mid rows behind the caller's, same
 * pitch) and the side rows live in a buffer of their own (int32, their own pitch). */
static bool stereo_on(const flacmi_frame_params* fp) { return fp->reserved[1] == FLACMI_STEREO_BEST; }

/* FLACMI_FLAG_SIZE_CHOICE at the host entry points: the written width is the stream's (a copy of
 * the parameters with reserved[2] filled, `out`); not with the wasted-bits mode, where it is per unit */
static int size_choice_params(const flacmi_params* p, const flacmi_frame_params* fp, flacmi_params* out) {
    *out = *p;
    if (!(p->reserved[1] & FLACMI_FLAG_SIZE_CHOICE)) return 0;
    if (fp->reserved0 & FLACMI_FRAME_WASTED)
        return fail(FLACMI_E_INVALID, "FLACMI_FLAG_SIZE_CHOICE does not combine with FLACMI_FRAME_WASTED");
    if (p->reserved[2] != 0 && p->reserved[2] != fp->sample_size)
        return fail(FLACMI_E_INVALID, "FLACMI_FLAG_SIZE_CHOICE: reserved[2] = %d disagrees with sample_size %d",
                    p->reserved[2], fp->sample_size);
    out->reserved[2] = fp->sample_size;
    return 0;
}
static size_t stereo_out_units(const flacmi_frame_params* fp, size_t nu) { return stereo_on(fp) ? 2 * nu : nu; }
static size_t stereo_sample_rows(const flacmi_frame_params* fp, size_t nu) { return stereo_on(fp) ? nu + nu / 2 : nu; }
static const void* stereo_mid(const flacmi_batch& db) {
    return (const char*)db.samples + (size_t)db.n_units * db.unit_stride * db.sample_bytes;
}

/* the *_device entry points' caller owns a layout of 2 units a frame */
static int no_stereo(const flacmi_frame_params* fp) {
    if (fp->reserved[1] != FLACMI_STEREO_OFF)
        return fail(FLACMI_E_INVALID, "the stereo mode (reserved[1]) is honoured by flacmi_encode_host and "
                                      "flacmi_encode_pipeline only");
    return 0;
}

/* k_stereo_rows, then three analyses into the one set of outputs `o`: the caller's 2 F units of
 * db (device rows), the F mid units and the F side units (an int32 batch, one bit wider); two
 * tail units become one tail mid unit and one tail side unit */
static int stereo_analyze(flacmi_ctx* ctx, const flacmi_batch& db, const flacmi_params* params,
                          const flacmi_outputs& o, DevBuf& side, hipStream_t s, bool allow_overlap) {
    const int64_t F = db.n_units / 2;
    const int64_t side_stride = row_pitch(db.block_len, 4);
    if (int rc = ensure_buf(side, (size_t)F * side_stride * sizeof(int32_t))) return rc;
    HIP_TRY(launch_stereo_rows(db.samples, db.sample_bytes, db.unit_stride, F, db.block_len, db.tail_len,
                               db.n_tail_units != 0, const_cast<void*>(stereo_mid(db)), db.unit_stride, (int32_t*)side.p,
                               side_stride, s));
    flacmi_batch bm = db;
    bm.samples = stereo_mid(db);
    bm.n_units = F;
    bm.n_tail_units = db.n_tail_units ? 1 : 0;
    flacmi_batch bs = bm;
    bs.samples = side.p;
    bs.sample_bytes = 4;
    bs.sample_bits = db.sample_bits + 1;
    bs.unit_stride = side_stride;
    const flacmi_batch* batches[3] = {&db, &bm, &bs};
    const int64_t unit0[3] = {0, 2 * F, 3 * F};
    /* FLACMI_FLAG_SIZE_CHOICE: the side rows are written one bit wider than the caller's and the mid rows */
    flacmi_params side_params = *params;
    if ((params->reserved[1] & FLACMI_FLAG_SIZE_CHOICE) && params->reserved[2]) side_params.reserved[2] += 1;
    const flacmi_params* const caller_params = params;
    for (int i = 0; i < 3; ++i) {
        params = i == 2 ? &side_params : caller_params;
        flacmi_outputs oi = o;
        oi.meta = o.meta + unit0[i];
        oi.rice_params = o.rice_params + unit0[i] * o.params_stride;
        oi.residual = (char*)o.residual + (size_t)unit0[i] * o.residual_stride * o.residual_bytes;
        if (int rc = validate(batches[i], params, &oi)) return rc;
        if (int rc = analyze_device_impl(ctx, batches[i], params, &oi, s, allow_overlap)) return rc;
    }
    return 0;
}

/* the frame writer's view of it: the choice array (one per context or pipeline slot), the mid and
 * side rows; before own_sub_kind */
static int stereo_args(const flacmi_frame_params* fp, const flacmi_batch& db, DevBuf& side, DevBuf& choice,
                       FrameArgs& a) {
    if (!stereo_on(fp)) return 0;
    if (int rc = ensure_buf(choice, sizeof(StereoChoice) * (size_t)a.n_frames)) return rc;
    a.choice = (StereoChoice*)choice.p;
    a.mid = stereo_mid(db);
    a.mid_stride = db.unit_stride;
    a.side = (const int32_t*)side.p;
    a.side_stride = row_pitch(db.block_len, 4);
    return 0;
}

/* ---- wasted-bits mode (FLACMI_FRAME_WASTED) at the host entry points ----------------------
 * The host entry points own their device copy of the rows: k_wasted_rows shifts it in place, once
 * per copy (a second run on shifted rows would find w = 0 and lose the shift), before the analysis,
 * which then sees the units x >> w; the wasted array is the context's or the pipeline slot's. */
static bool wasted_on(const flacmi_frame_params* fp) { return (fp->reserved0 & FLACMI_FRAME_WASTED) != 0; }
static int no_wasted(const flacmi_frame_params* fp) {
    if (wasted_on(fp))
        return fail(FLACMI_E_INVALID, "the frame flag FLACMI_FRAME_WASTED (reserved0) is honoured by flacmi_encode_host and "
                                      "flacmi_encode_pipeline only");
    return 0;
}
static int wasted_shift(const flacmi_frame_params* fp, const flacmi_batch& db, DevBuf& buf, hipStream_t s) {
    if (!wasted_on(fp)) return 0;
    /* the kernel runs ahead of the analysis' own validation of the batch */
    if ((db.sample_bytes != 2 && db.sample_bytes != 4) || db.sample_bits < 1 || db.sample_bits > 8 * db.sample_bytes)
        return fail(FLACMI_E_INVALID, "sample_bytes must be 2 or 4 and sample_bits fit them");
    if (db.n_tail_units > 0 && (db.tail_len < 1 || db.tail_len > db.block_len))
        return fail(FLACMI_E_INVALID, "tail_len out of range");
    if (int rc = ensure_buf(buf, sizeof(int32_t) * (size_t)db.n_units)) return rc;
    const int bits = db.sample_bits < fp->sample_size ? db.sample_bits : fp->sample_size;
    HIP_TRY(launch_wasted_rows(db.samples, db.sample_bytes, db.unit_stride, db.n_units, db.block_len,
                               db.n_tail_units ? db.tail_len : db.block_len, db.n_tail_units, bits,
                               const_cast<void*>(db.samples), db.unit_stride, (int32_t*)buf.p, s));
    return 0;
}
static void wasted_args(const flacmi_frame_params* fp, DevBuf& buf, FrameArgs& a) {
    if (wasted_on(fp)) a.wasted = (const int32_t*)buf.p;
}

/* the k_pack32 -> k_pack hand-off list (count word + one index per frame) */
static int pack_lists(flacmi_ctx* ctx, FrameArgs& a) {
    if (int rc = ensure_buf(ctx->slow, sizeof(int64_t) * (size_t)(a.n_frames + 2))) return rc;
    a.slow_count = (unsigned long long*)ctx->slow.p;
    a.slow_list = (int64_t*)ctx->slow.p + 2;
    return 0;
}

static int frame_sizes_impl(flacmi_ctx* ctx, FrameArgs& a, int64_t* offsets, int32_t* status, hipStream_t s) {
    a.offsets = offsets;
    a.status = status;
    if (int rc = ensure_buf(ctx->scan, sizeof(int64_t) * (size_t)(frame_scan_blocks(a.n_frames) + 1))) return rc;
    HIP_TRY(launch_frame_sizes(a, (int64_t*)ctx->scan.p, s));
    return 0;
}

extern "C" {

int flacmi_frame_sizes_device(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_frame_params* fp,
                              const flacmi_unit_meta* meta, const int32_t* rice_params, int64_t params_stride,
                              int64_t* frame_offsets, int32_t* frame_status, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    int64_t nf = 0;
    if (int rc = validate_frames(batch, fp, &nf)) return rc;
    if (int rc = no_stereo(fp)) return rc;
    if (int rc = no_wasted(fp)) return rc;
    if (!meta || !rice_params || !frame_offsets || !frame_status) return fail(FLACMI_E_INVALID, "null buffer");
    if (int rc = set_device(ctx)) return rc;
    if (nf == 0) {
        HIP_TRY(hipMemsetAsync(frame_offsets, 0, sizeof(int64_t), (hipStream_t)stream));
        return 0;
    }
    FrameArgs a = frame_args(ctx, batch, fp, meta, rice_params, params_stride, nf);
    if (int rc = caller_sub_kind(fp, a)) return rc;
    return frame_sizes_impl(ctx, a, frame_offsets, frame_status, (hipStream_t)stream);
}

int flacmi_pack_frames_device(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_frame_params* fp,
                              const flacmi_unit_meta* meta, const int32_t* rice_params, int64_t params_stride,
                              const void* residual, int32_t residual_bytes, int64_t residual_stride,
                              const int64_t* frame_offsets, int32_t* frame_status, uint8_t* out,
                              int64_t out_capacity, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    int64_t nf = 0;
    if (int rc = validate_frames(batch, fp, &nf)) return rc;
    if (int rc = no_stereo(fp)) return rc;
    if (int rc = no_wasted(fp)) return rc;
    if (!meta || !rice_params || !residual || !frame_offsets || !frame_status || (!out && out_capacity > 0))
        return fail(FLACMI_E_INVALID, "null buffer");
    if (residual_bytes != 4 && residual_bytes != 8) return fail(FLACMI_E_INVALID, "residual_bytes must be 4 or 8");
    if (residual_stride < batch->block_len) return fail(FLACMI_E_INVALID, "residual_stride < block_len");
    if (((uintptr_t)out & 3) != 0) return fail(FLACMI_E_INVALID, "out must be 4-byte aligned");
    if (nf == 0) return 0;
    if (int rc = set_device(ctx)) return rc;
    FrameArgs a = frame_args(ctx, batch, fp, meta, rice_params, params_stride, nf);
    if (int rc = caller_sub_kind(fp, a)) return rc;
    a.residual = residual;
    a.residual_bytes = residual_bytes;
    a.residual_stride = residual_stride;
    a.offsets = const_cast<int64_t*>(frame_offsets);
    a.status = frame_status;
    a.out = out;
    a.capacity = out_capacity;
    if (int rc = pack_lists(ctx, a)) return rc;
    HIP_TRY(launch_pack(a, (hipStream_t)stream));
    return 0;
}

int flacmi_stereo_rows_device(flacmi_ctx* ctx, const flacmi_batch* lr, void* mid, int64_t mid_stride, int32_t* side,
                              int64_t side_stride, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (!lr || !mid || !side) return fail(FLACMI_E_INVALID, "null argument");
    if (lr->sample_bytes != 2 && lr->sample_bytes != 4) return fail(FLACMI_E_INVALID, "sample_bytes must be 2 or 4");
    if (lr->n_units < 0 || lr->n_units % 2 != 0) return fail(FLACMI_E_INVALID, "n_units must be even (left, right rows)");
    if (lr->n_tail_units != 0 && (lr->n_tail_units != 2 || lr->n_units < 2))
        return fail(FLACMI_E_INVALID, "the short last frame must hold exactly 2 tail units");
    if (lr->block_len < 1 || lr->block_len > FLACMI_MAX_BLOCK) return fail(FLACMI_E_INVALID, "block_len out of range");
    if (lr->n_tail_units > 0 && (lr->tail_len < 1 || lr->tail_len > lr->block_len))
        return fail(FLACMI_E_INVALID, "tail_len out of range");
    if (lr->n_units == 0) return 0;
    if (!lr->samples) return fail(FLACMI_E_INVALID, "null argument");
    if (lr->unit_stride < lr->block_len || mid_stride < lr->block_len || side_stride < lr->block_len)
        return fail(FLACMI_E_INVALID, "a row pitch is below block_len");
    if ((lr->unit_stride * lr->sample_bytes) % 16 != 0 || (mid_stride * lr->sample_bytes) % 16 != 0 ||
        (side_stride * 4) % 16 != 0 || ((uintptr_t)lr->samples | (uintptr_t)mid | (uintptr_t)side) % 16 != 0)
        return fail(FLACMI_E_INVALID, "rows must be 16-byte aligned and every pitch a multiple of 16 bytes");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(launch_stereo_rows(lr->samples, lr->sample_bytes, lr->unit_stride, lr->n_units / 2, lr->block_len,
                               lr->tail_len, lr->n_tail_units != 0, mid, mid_stride, side, side_stride,
                               (hipStream_t)stream));
    return 0;
}

int flacmi_wasted_rows_device(flacmi_ctx* ctx, const flacmi_batch* in, void* out_rows, int64_t out_stride,
                              int32_t* wasted, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (!in || !out_rows || !wasted) return fail(FLACMI_E_INVALID, "null argument");
    if (in->sample_bytes != 2 && in->sample_bytes != 4) return fail(FLACMI_E_INVALID, "sample_bytes must be 2 or 4");
    if (in->sample_bits < 1 || in->sample_bits > 8 * in->sample_bytes)
        return fail(FLACMI_E_INVALID, "sample_bits out of range for the row type");
    if (in->n_units < 0 || in->n_tail_units < 0 || in->n_tail_units > in->n_units)
        return fail(FLACMI_E_INVALID, "n_units / n_tail_units out of range");
    if (in->block_len < 1 || in->block_len > FLACMI_MAX_BLOCK) return fail(FLACMI_E_INVALID, "block_len out of range");
    if (in->n_tail_units > 0 && (in->tail_len < 1 || in->tail_len > in->block_len))
        return fail(FLACMI_E_INVALID, "tail_len out of range");
    if (in->n_units == 0) return 0;
    if (!in->samples) return fail(FLACMI_E_INVALID, "null argument");
    if (in->unit_stride < in->block_len || out_stride < in->block_len)
        return fail(FLACMI_E_INVALID, "a row pitch is below block_len");
    if ((in->unit_stride * in->sample_bytes) % 16 != 0 || (out_stride * in->sample_bytes) % 16 != 0 ||
        ((uintptr_t)in->samples | (uintptr_t)out_rows) % 16 != 0 || (uintptr_t)wasted % 4 != 0)
        return fail(FLACMI_E_INVALID, "rows must be 16-byte aligned and every pitch a multiple of 16 bytes");
    if (out_rows == in->samples && out_stride != in->unit_stride)
        return fail(FLACMI_E_INVALID, "in place the output pitch is the input pitch");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(launch_wasted_rows(in->samples, in->sample_bytes, in->unit_stride, in->n_units, in->block_len,
                               in->tail_len, in->n_tail_units, in->sample_bits, out_rows, out_stride, wasted,
                               (hipStream_t)stream));
    return 0;
}

int flacmi_decode_frames_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                                const int64_t* frame_offsets, int64_t n_frames,
                                const flacmi_decode_params* dp, const flacmi_batch* expect,
                                int32_t* samples_out, int64_t out_stride, int32_t* frame_status,
                                int64_t* frame_mismatch, void* stream) {
    return flacmi_decode_frames_end_device(ctx, stream_data, stream_bytes, frame_offsets, n_frames, dp, expect,
                                           samples_out, out_stride, frame_status, frame_mismatch, nullptr, stream);
}

/* flacmi_decode_params.reserved0: enum flacmi_decode_flags bits */
static int decode_flags_ok(const flacmi_decode_params* dp) {
    if (dp->reserved0 & ~FLACMI_DECODE_WASTED_SPEC)
        return fail(FLACMI_E_INVALID, "unknown decode flag bits %#x (reserved0)", (unsigned)dp->reserved0);
    return 0;
}

static int decode_frames_impl(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                              const int64_t* frame_offsets, int64_t n_frames, const flacmi_decode_params* dp,
                              const flacmi_batch* expect, int32_t* samples_out, int64_t out_stride,
                              int32_t* frame_status, int64_t* frame_mismatch, int64_t* frame_end, bool general,
                              void* stream, const int64_t* frame_limit = nullptr);

int flacmi_decode_frames_end_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                                    const int64_t* frame_offsets, int64_t n_frames,
                                    const flacmi_decode_params* dp, const flacmi_batch* expect,
                                    int32_t* samples_out, int64_t out_stride, int32_t* frame_status,
                                    int64_t* frame_mismatch, int64_t* frame_end, void* stream) {
    return decode_frames_impl(ctx, stream_data, stream_bytes, frame_offsets, n_frames, dp, expect, samples_out,
                              out_stride, frame_status, frame_mismatch, frame_end, false, stream);
}

/* general: every frame through the general decoder kernel, as knob FLACMI_DECODE_GENERIC;
 * frame_limit (device, [n_frames], the batch decoder): the end of each frame's own stream */
static int decode_frames_impl(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                              const int64_t* frame_offsets, int64_t n_frames, const flacmi_decode_params* dp,
                              const flacmi_batch* expect, int32_t* samples_out, int64_t out_stride,
                              int32_t* frame_status, int64_t* frame_mismatch, int64_t* frame_end, bool general,
                              void* stream, const int64_t* frame_limit) {
    if (!ctx || !dp) return fail(FLACMI_E_INVALID, "null argument");
    if (n_frames < 0 || stream_bytes < 0) return fail(FLACMI_E_INVALID, "negative size");
    if (n_frames == 0) return 0;
    if (!stream_data || !frame_offsets || !frame_status || !frame_mismatch) return fail(FLACMI_E_INVALID, "null buffer");
    if (((uintptr_t)stream_data & 3) != 0) return fail(FLACMI_E_INVALID, "stream_data must be 4-byte aligned");
    if (dp->channels < 1 || dp->channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (dp->sample_size < 4 || dp->sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 4..32");
    if (int rc = decode_flags_ok(dp)) return rc;
    if (samples_out && (out_stride < 1 || (out_stride & 3) != 0 || ((uintptr_t)samples_out & 15) != 0))
        return fail(FLACMI_E_INVALID, "samples_out rows must be 16-byte aligned (out_stride a multiple of 4)");
    if (expect) {
        if (expect->sample_bytes != 2 && expect->sample_bytes != 4) return fail(FLACMI_E_INVALID, "expect: sample_bytes 2 or 4");
        if (expect->n_units != n_frames * dp->channels) return fail(FLACMI_E_INVALID, "expect: n_units != n_frames * channels");
        if (expect->unit_stride < expect->block_len) return fail(FLACMI_E_INVALID, "expect: unit_stride < block_len");
        if (expect->n_tail_units && expect->tail_len > expect->block_len) return fail(FLACMI_E_INVALID, "expect: tail_len > block_len");
    }
    if (int rc = set_device(ctx)) return rc;
    /* workspace: decorr codes [n_frames] i32, then two deferred-frame lists (an 8 B count and
     * [n_frames] i64 each) */
    const size_t dlist = (sizeof(int32_t) * (size_t)n_frames + 15) & ~(size_t)15;
    const size_t dl2 = dlist + 16 + sizeof(int64_t) * (size_t)n_frames; /* the second list */
    if (int rc = ensure_buf(ctx->dec, dl2 + 16 + sizeof(int64_t) * (size_t)n_frames)) return rc;
    DecodeArgs a{};
    a.words = reinterpret_cast<const uint32_t*>(stream_data);
    a.stream_bytes = stream_bytes;
    a.n_words = (stream_bytes + 3) / 4;
    a.offsets = frame_offsets;
    a.n_frames = n_frames;
    a.channels = dp->channels;
    a.sample_size = dp->sample_size;
    a.first_frame = dp->first_frame;
    a.check_crc = dp->check_crc;
    a.wasted_spec = (dp->reserved0 & FLACMI_DECODE_WASTED_SPEC) != 0;
    if (expect) {
        a.expect = expect->samples;
        a.expect_stride = expect->unit_stride;
        a.expect_bytes = expect->sample_bytes;
        a.expect_vec = ((uintptr_t)expect->samples & 15) == 0 && ((expect->unit_stride * expect->sample_bytes) & 15) == 0;
        a.block_len = expect->block_len;
        a.tail_len = expect->n_tail_units ? expect->tail_len : expect->block_len;
        a.n_units = expect->n_units;
        a.n_tail_units = expect->n_tail_units;
    }
    a.out = samples_out;
    a.out_stride = out_stride;
    a.status = frame_status;
    a.mismatch = frame_mismatch;
    a.decorr = (int32_t*)ctx->dec.p;
    a.defer_count = (unsigned long long*)((char*)ctx->dec.p + dlist);
    a.defer_list = (int64_t*)((char*)ctx->dec.p + dlist + 16);
    a.defer2_count = (unsigned long long*)((char*)ctx->dec.p + dl2);
    a.defer2_list = (int64_t*)((char*)ctx->dec.p + dl2 + 16);
    a.defer_all = general || knob(kKnobDecodeGeneric) != 0;
    a.crc_slice = ctx->d_crc;
    a.frame_end = frame_end;
    a.frame_limit = frame_limit;
    HIP_TRY(launch_decode(a, (hipStream_t)stream));
    return 0;
}

/* ---- stream decoder ------------------------------------------------------------------ */
int32_t flacmi_index_tile_bytes(void) { return kIndexTile; }

int flacmi_index_frames_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                               int64_t first_byte, flacmi_frame_candidate* table, int64_t capacity,
                               int64_t* count, void* stream) {
    if (!ctx || !count) return fail(FLACMI_E_INVALID, "null argument");
    if (stream_bytes < 0 || first_byte < 0 || capacity < 0) return fail(FLACMI_E_INVALID, "negative size");
    if (stream_bytes > 0 && !stream_data) return fail(FLACMI_E_INVALID, "null buffer");
    if (capacity > 0 && !table) return fail(FLACMI_E_INVALID, "null table");
    if (((uintptr_t)stream_data & 3) != 0) return fail(FLACMI_E_INVALID, "stream_data must be 4-byte aligned");
    if (((uintptr_t)table & 7) != 0 || ((uintptr_t)count & 7) != 0)
        return fail(FLACMI_E_INVALID, "table and count must be 8-byte aligned");
    if (int rc = set_device(ctx)) return rc;
    IndexArgs a{};
    a.base = stream_data;
    a.bytes = stream_bytes;
    a.first = first_byte;
    a.mis = (int32_t)((uintptr_t)stream_data & 15);
    a.n_tiles = stream_bytes > 0 ? (a.mis + stream_bytes + kIndexTile - 1) / kIndexTile : 0;
    if (a.n_tiles > 0x7FFFFFFF) return fail(FLACMI_E_UNSUPPORTED, "stream of %lld bytes: index it in parts", (long long)stream_bytes);
    a.table = table;
    a.capacity = capacity;
    a.count = count;
    /* workspace: group bases i64, then tile bases [n_tiles] i32 and tile counts [n_tiles + 3] i32 */
    const size_t ng = (size_t)index_scan_groups(a.n_tiles);
    if (int rc = ensure_buf(ctx->idx, 8 * ng + 8 * (size_t)a.n_tiles + 32)) return rc;
    a.group_base = (int64_t*)ctx->idx.p;
    a.tile_base = (int32_t*)((char*)ctx->idx.p + 8 * ng);
    a.tile_count = a.tile_base + a.n_tiles;
    HIP_TRY(launch_index(a, (hipStream_t)stream));
    return 0;
}

int flacmi_pcm_out_device(flacmi_ctx* ctx, const flacmi_pcm_frame* frames, int64_t n_frames, int32_t channels,
                          int32_t bytes_per_sample, int32_t mode, uint8_t* out, int64_t out_capacity,
                          int32_t* frame_status, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null argument");
    if (n_frames < 0 || out_capacity < 0) return fail(FLACMI_E_INVALID, "negative size");
    if (channels < 1 || channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (mode != FLACMI_PCM_PACKED && mode != FLACMI_PCM_RAW32) return fail(FLACMI_E_INVALID, "mode must be a flacmi_pcm_mode");
    if (mode == FLACMI_PCM_PACKED && (bytes_per_sample < 1 || bytes_per_sample > 4))
        return fail(FLACMI_E_INVALID, "bytes_per_sample must be 1..4");
    if (n_frames == 0) return 0;
    if (!frames || !out || !frame_status) return fail(FLACMI_E_INVALID, "null buffer");
    if (((uintptr_t)out & 3) != 0 || ((uintptr_t)frames & 7) != 0) return fail(FLACMI_E_INVALID, "out must be 4-byte aligned");
    if (n_frames > 0x7FFFFFFF) return fail(FLACMI_E_UNSUPPORTED, "more than 2^31 - 1 frames in one call");
    if (int rc = set_device(ctx)) return rc;
    PcmArgs a{};
    a.frames = frames;
    a.n_frames = n_frames;
    a.channels = channels;
    a.bytes_per_sample = mode == FLACMI_PCM_RAW32 ? 4 : bytes_per_sample;
    a.raw = mode == FLACMI_PCM_RAW32;
    a.out = out;
    a.capacity = out_capacity;
    a.status = frame_status;
    HIP_TRY(launch_pcm(a, (hipStream_t)stream));
    return 0;
}

int flacmi_units_out_device(flacmi_ctx* ctx, const flacmi_pcm_frame* frames, int64_t n_frames, int32_t channels,
                            int64_t first_sample, int32_t block_len, int64_t n_blocks, int32_t tail_len,
                            int32_t sample_size, void* units, int32_t sample_bytes, int64_t unit_stride,
                            int32_t* frame_status, uint32_t* width, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null argument");
    if (n_frames < 0 || n_blocks < 0 || first_sample < 0) return fail(FLACMI_E_INVALID, "negative size");
    if (channels < 1 || channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (block_len < 1 || block_len > FLACMI_MAX_BLOCK) return fail(FLACMI_E_INVALID, "block_len out of range");
    if (tail_len < 0 || tail_len >= block_len) return fail(FLACMI_E_INVALID, "tail_len must be 0..block_len - 1");
    if (sample_bytes != 2 && sample_bytes != 4) return fail(FLACMI_E_INVALID, "sample_bytes must be 2 or 4");
    if (sample_size < 4 || sample_size > 8 * sample_bytes)
        return fail(FLACMI_E_INVALID, "sample_size must be 4..%d for %d-byte rows", 8 * sample_bytes, sample_bytes);
    if (unit_stride < block_len || (unit_stride * sample_bytes) % 16 != 0)
        return fail(FLACMI_E_INVALID, "unit_stride must hold block_len samples and be a multiple of 16 bytes");
    if (!width || (n_frames > 0 && (!frames || !frame_status))) return fail(FLACMI_E_INVALID, "null buffer");
    if (((uintptr_t)frames & 7) != 0 || ((uintptr_t)units & 15) != 0 || (((uintptr_t)frame_status | (uintptr_t)width) & 3) != 0)
        return fail(FLACMI_E_INVALID, "units must be 16-byte aligned, frames 8-byte, frame_status and width 4-byte");
    const int64_t blocks = n_blocks + (tail_len > 0 ? 1 : 0);
    if (blocks > 0x7FFFFFFF / channels) return fail(FLACMI_E_UNSUPPORTED, "more than 2^31 - 1 units in one call");
    if (blocks > 0 && !units) return fail(FLACMI_E_INVALID, "null units");
    if (int rc = set_device(ctx)) return rc;
    UnitsArgs a{};
    a.frames = frames;
    a.n_frames = n_frames;
    a.channels = channels;
    a.block_len = block_len;
    a.tail_len = tail_len;
    a.sample_size = sample_size;
    a.s0 = first_sample;
    a.n_blocks = n_blocks;
    a.units = units;
    a.stride = unit_stride;
    a.status = frame_status;
    a.width = width;
    HIP_TRY(launch_units(a, sample_bytes, (hipStream_t)stream));
    return 0;
}

int flacmi_planar_out_device(flacmi_ctx* ctx, const flacmi_pcm_frame* frames, int64_t n_frames, int64_t n_streams,
                             int32_t channels, const int64_t* lengths, int32_t sample_size, int32_t elem, void* out,
                             int64_t pitch, int32_t* frame_status, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null argument");
    if (n_frames < 0 || n_streams < 0 || pitch < 0) return fail(FLACMI_E_INVALID, "negative size");
    if (channels < 1 || channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (elem != FLACMI_PLANAR_INT16 && elem != FLACMI_PLANAR_INT32 && elem != FLACMI_PLANAR_FLOAT32)
        return fail(FLACMI_E_INVALID, "elem must be a flacmi_planar_elem");
    if (sample_size < 4 || sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 4..32");
    const int sb = elem == FLACMI_PLANAR_INT16 ? 2 : 4;
    if ((pitch * sb) % 16 != 0) return fail(FLACMI_E_INVALID, "pitch must be a multiple of 16 bytes");
    if (n_frames > 0 && (!frames || !frame_status)) return fail(FLACMI_E_INVALID, "null buffer");
    if (((uintptr_t)frames & 7) != 0 || ((uintptr_t)out & 15) != 0 || ((uintptr_t)frame_status & 3) != 0 || ((uintptr_t)lengths & 7) != 0)
        return fail(FLACMI_E_INVALID, "out must be 16-byte aligned, frames and lengths 8-byte, frame_status 4-byte");
    if (n_frames > 0x7FFFFFFF || n_streams > 0x7FFFFFFF) return fail(FLACMI_E_UNSUPPORTED, "more than 2^31 - 1 frames or streams in one call");
    if (n_streams == 0 || pitch == 0) return 0;
    if (!out) return fail(FLACMI_E_INVALID, "null out");
    const int64_t per = 256 * (16 / sb), tiles = (pitch + per - 1) / per;
    if (tiles > 0x7FFFFFFF / (n_streams * channels)) return fail(FLACMI_E_UNSUPPORTED, "more than 2^31 - 1 workgroups: pass fewer streams");
    if (int rc = set_device(ctx)) return rc;
    PlanarArgs a{};
    a.frames = frames;
    a.n_frames = n_frames;
    a.n_streams = n_streams;
    a.channels = channels;
    a.sample_size = sample_size;
    a.lengths = lengths;
    a.out = out;
    a.pitch = pitch;
    a.status = frame_status;
    HIP_TRY(launch_planar(a, elem, (hipStream_t)stream));
    return 0;
}

static inline bool walk_ref_error(int32_t st) { return st != 0 && (st & 0xFFFF) != FLACMI_STATUS_VERIFY; }

int flacmi_host_chain_walk(const flacmi_frame_candidate* table, int64_t n_candidates, const int32_t* status,
                           const int64_t* frame_end, int64_t stream_bytes, int32_t final_chunk, flacmi_walk* w,
                           flacmi_chain_frame* chain, int64_t chain_capacity) {
    (void)final_chunk; /* an EOFError frame leaves w->pos at its start either way: the final chunk's caller ends
                          the stream there, any other caller carries the tail over */
    if (!w || n_candidates < 0 || stream_bytes < 0 || chain_capacity < 0) return fail(FLACMI_E_INVALID, "bad argument");
    if (n_candidates > 0 && (!table || !status || !frame_end)) return fail(FLACMI_E_INVALID, "null table");
    if (chain_capacity > 0 && !chain) return fail(FLACMI_E_INVALID, "null chain");
    if (w->pos < 0 || w->n_chain < 0 || w->n_chain > chain_capacity) return fail(FLACMI_E_INVALID, "bad walk state");
    if (w->state == FLACMI_WALK_DONE || w->state == FLACMI_WALK_STOPPED) return 0;
    bool probed = w->state == FLACMI_WALK_PROBE;
    for (;;) {
        const int64_t pos = w->pos;
        if (pos >= stream_bytes) {
            w->state = FLACMI_WALK_DONE;
            return 0;
        }
        /* the candidate at exactly pos */
        int64_t lo = 0, hi = n_candidates;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (table[mid].offset < pos) lo = mid + 1;
            else hi = mid;
        }
        const int64_t k = (lo < n_candidates && table[lo].offset == pos) ? lo : -1;
        int32_t st;
        int64_t end;
        const bool was_probed = probed;
        if (probed) {
            st = w->probe_status;
            end = w->probe_end;
            probed = false;
            if (!walk_ref_error(st) && end <= pos) { /* not parsed to its end */
                w->state = FLACMI_WALK_STOPPED;
                w->stop_status = st ? st : ((FLACMI_DSITE_FRAME_END << 16) | FLACMI_STATUS_VERIFY);
                return 0;
            }
        } else if (k < 0) {
            w->state = FLACMI_WALK_PROBE;
            return 0;
        } else {
            st = status[k];
            end = st == 0 ? (k + 1 < n_candidates ? table[k + 1].offset : stream_bytes) : frame_end[k];
            if (!walk_ref_error(st) && end <= pos) { /* a block larger than the first pass's rows */
                w->state = FLACMI_WALK_PROBE;
                return 0;
            }
        }
        if (walk_ref_error(st)) {
            if ((st & 0xFFFF) == FLACMI_STATUS_EOF) {
                w->state = FLACMI_WALK_DONE;
            } else {
                w->state = FLACMI_WALK_STOPPED;
                w->stop_status = st;
            }
            return 0;
        }
        if (w->n_chain >= chain_capacity) {
            w->state = FLACMI_WALK_FULL;
            if (was_probed) { /* keep the probe's answer for the next call */
                w->state = FLACMI_WALK_PROBE;
                w->probe_status = st;
                w->probe_end = end;
                return fail(FLACMI_E_NOMEM, "chain_capacity reached on a probed frame: pass room for one more");
            }
            return 0;
        }
        flacmi_chain_frame& c = chain[w->n_chain++];
        c.offset = pos;
        c.end = end;
        c.candidate = k;
        /* a probed frame's rows are the caller's to decode again: never final */
        c.status = (was_probed && st == 0) ? ((FLACMI_DSITE_FRAME_END << 16) | FLACMI_STATUS_VERIFY) : st;
        c.reserved0 = 0;
        w->pos = end;
        w->state = FLACMI_WALK_RUN;
    }
}

namespace {
struct ScopedDev { /* device scratch of one flacmi_decode_stream_host call */
    void* p = nullptr;
    ~ScopedDev() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) {
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) {
            p = nullptr;
            return fail(FLACMI_E_NOMEM, "hipMalloc of %zu bytes failed", bytes);
        }
        return 0;
    }
};
}  // namespace

/* Steps 1 to 5 of flacmi_decode_stream_host (copy in, index, pass 1, the chain walk with its
 * probes, pass 2), shared with flacmi_recompress_host: the chain's first nc frames are decoded,
 * frame i's rows are pass 2's (row2[i] >= 0: rows2 at stride2) or pass 1's (its candidate's, in
 * ctx->sd_rows at stride1); stop is the status word of the frame at pos, or 0.
 *
 * flacmi_decode_batch_host runs the same steps once over many whole streams packed back to
 * back (seg[0 .. nseg] their bounds): every stream's first byte joins the candidates, so no
 * proposed end lies past the frame's own stream; the walk runs once per stream over its slice of
 * the table and leaves stream s's frames in chain[segs[s].c0 ..) with its own nc, stop and pos;
 * the general decoder gets each frame's stream end (DecodeArgs.frame_limit).  Without seg the
 * launches are the single stream's, in its order. */
namespace {
struct StreamFrames {
    struct Seg {
        int64_t c0 = 0, nc = 0, pos = 0, probes = 0, n2 = 0;
        int32_t stop = 0;
    };
    std::vector<flacmi_chain_frame> chain;
    std::vector<int32_t> bsz;
    std::vector<int64_t> row2;
    std::vector<Seg> segs; /* the batch decoder's streams */
    ScopedDev rows2;
    int64_t nc = 0, n2 = 0, stride1 = 4, stride2 = 4, pos = 0, candidates = 0, probes = 0;
    int32_t stop = 0;
};
}  // namespace

static void batch_invalidate(flacmi_ctx* ctx);

static int stream_frames(flacmi_ctx* ctx, const uint8_t* data, int64_t bytes, int64_t first_byte,
                         const flacmi_decode_params* dp, int32_t max_block_size, int32_t final_chunk, StreamFrames& h,
                         const int64_t* seg = nullptr, int64_t nseg = 0) {
    hipStream_t s = ctx->stream;
    const int ch = dp->channels;
    const bool batch = seg != nullptr;
    flacmi_decode_params p1 = *dp;
    p1.first_frame = -1;
    batch_invalidate(ctx); /* a kept frame list points into the buffers this call reuses */

    /* 1. the chunk, 2. the index */
    if (int rc = ensure_buf(ctx->sd_data, (size_t)bytes + 32)) return rc;
    uint8_t* d_data = (uint8_t*)ctx->sd_data.p;
    HIP_TRY(hipMemcpyAsync(d_data, data, (size_t)bytes, hipMemcpyHostToDevice, s));
    int64_t cap = bytes / 512 + 1024, n = 0;
    for (;;) {
        if (int rc = ensure_buf(ctx->sd_table, sizeof(flacmi_frame_candidate) * (size_t)cap + 16)) return rc;
        int64_t* d_count = (int64_t*)ctx->sd_table.p;
        if (int rc = flacmi_index_frames_device(ctx, d_data, bytes, first_byte,
                                                (flacmi_frame_candidate*)((char*)ctx->sd_table.p + 16), cap, d_count, s))
            return rc;
        HIP_TRY(hipMemcpyAsync(&n, d_count, sizeof(n), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n <= cap) break;
        cap = n;
    }
    h.candidates = n;
    std::vector<flacmi_frame_candidate> table((size_t)n);
    if (n) HIP_TRY(hipMemcpy(table.data(), (char*)ctx->sd_table.p + 16, sizeof(flacmi_frame_candidate) * (size_t)n, hipMemcpyDeviceToHost));

    /* the batch: every stream's first byte is a candidate, listed or not; seg_k[s] is the table
     * index of stream s's first candidate, lim[k] the end of candidate k's stream */
    std::vector<int64_t> seg_k, lim;
    if (batch) {
        std::vector<flacmi_frame_candidate> merged;
        merged.reserve((size_t)(n + nseg));
        seg_k.assign((size_t)nseg + 1, 0);
        int64_t k = 0;
        for (int64_t g = 0; g < nseg; ++g) {
            const int64_t b = seg[g], e = seg[g + 1];
            seg_k[(size_t)g] = (int64_t)merged.size();
            if (b == e) continue;
            if (!(k < n && table[(size_t)k].offset == b)) {
                flacmi_frame_candidate c{};
                if (e - b >= 2 && data[b] == 0xFF && (data[b + 1] & 0xFE) == 0xF8 && parse_header(data + b, e - b, 0, false, c)) {
                    const int32_t bs = c.block_size;
                    c = flacmi_frame_candidate{};
                    c.block_size = bs;
                }
                c.offset = b;
                merged.push_back(c);
                lim.push_back(e);
            }
            for (; k < n && table[(size_t)k].offset < e; ++k) {
                merged.push_back(table[(size_t)k]);
                lim.push_back(e);
            }
        }
        seg_k[(size_t)nseg] = (int64_t)merged.size();
        table.swap(merged);
        n = (int64_t)table.size();
    }

    /* 3. pass 1: every candidate, proposed to end at the next one */
    int64_t stride1 = max_block_size;
    if (stride1 == 0)
        for (const auto& c : table) stride1 = std::max<int64_t>(stride1, c.block_size);
    stride1 = std::max<int64_t>(4, (stride1 + 3) & ~(int64_t)3);
    const size_t rows1 = sizeof(int32_t) * (size_t)n * ch * (size_t)stride1;
    if (rows1 > ((size_t)4 << 30))
        return fail(FLACMI_E_UNSUPPORTED, "%lld candidates of %lld-sample rows exceed 4 GiB: pass a smaller chunk", (long long)n, (long long)stride1);
    std::vector<int32_t> st1((size_t)n);
    std::vector<int64_t> end1((size_t)n);
    /* per-frame words: offsets [n + 1] i64, ends [n] i64, mismatches [n] i64, stream ends [n] i64 (the
     * batch), status [n] i32 */
    if (int rc = ensure_buf(ctx->sd_meta, 36 * (size_t)n + 64)) return rc;
    int64_t* d_off = (int64_t*)ctx->sd_meta.p;
    int64_t* d_end = d_off + n + 1;
    int64_t* d_mm = d_end + n;
    int64_t* d_lim = d_mm + n;
    int32_t* d_st = (int32_t*)(d_lim + n);
    if (n) {
        std::vector<int64_t> off((size_t)n + 1);
        for (int64_t k = 0; k < n; ++k) off[k] = table[k].offset;
        off[n] = bytes;
        if (int rc = ensure_buf(ctx->sd_rows, rows1)) return rc;
        HIP_TRY(hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, s));
        if (batch) HIP_TRY(hipMemcpyAsync(d_lim, lim.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
        if (int rc = decode_frames_impl(ctx, d_data, bytes, d_off, n, &p1, nullptr, (int32_t*)ctx->sd_rows.p, stride1, d_st, d_mm,
                                        d_end, false, s, batch ? d_lim : nullptr))
            return rc;
        HIP_TRY(hipMemcpyAsync(st1.data(), d_st, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(end1.data(), d_end, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }

    /* 4. the walk, once per stream; a probe decodes the one frame at w.pos into rows of the largest block */
    std::vector<flacmi_chain_frame>& chain = h.chain;
    chain.assign((size_t)n + 16, flacmi_chain_frame{});
    std::vector<StreamFrames::Seg>& segs = h.segs;
    const int64_t one[2] = {first_byte, bytes};
    if (!batch) seg = one, nseg = 1;
    segs.assign((size_t)nseg, StreamFrames::Seg{});
    ScopedDev probe_rows, probe_meta;
    constexpr int64_t kProbeStride = 65536;
    int64_t total = 0; /* chain frames of the streams before */
    for (int64_t g = 0; g < nseg; ++g) {
        StreamFrames::Seg& sg = segs[(size_t)g];
        const int64_t k0 = batch ? seg_k[(size_t)g] : 0, k1 = batch ? seg_k[(size_t)g + 1] : n, send = seg[g + 1];
        flacmi_walk w{};
        w.pos = seg[g];
        sg.c0 = total;
        for (;;) {
            if ((int64_t)chain.size() < total + 16) chain.resize(2 * chain.size() + 16);
            if (int rc = flacmi_host_chain_walk(table.data() + k0, k1 - k0, st1.data() + k0, end1.data() + k0, send, final_chunk, &w,
                                                chain.data() + total, (int64_t)chain.size() - total))
                return rc;
            if (w.state == FLACMI_WALK_FULL) {
                chain.resize(chain.size() * 2);
                w.state = FLACMI_WALK_RUN;
                continue;
            }
            if (w.state != FLACMI_WALK_PROBE) break;
            if ((int64_t)chain.size() - total == w.n_chain) chain.resize(chain.size() * 2);
            if (!probe_rows.p) {
                if (int rc = probe_rows.alloc(sizeof(int32_t) * (size_t)ch * kProbeStride)) return rc;
                if (int rc = probe_meta.alloc(64)) return rc;
            }
            int64_t* q_off = (int64_t*)probe_meta.p; /* offsets [2], end, mismatch, status */
            const int64_t off2[2] = {w.pos, send};
            HIP_TRY(hipMemcpyAsync(q_off, off2, sizeof(off2), hipMemcpyHostToDevice, s));
            int32_t k1s = 0;
            HIP_TRY(hipStreamSynchronize(s)); /* off2 is a stack array */
            /* FLACMI_DECODE_GENERIC semantics: the general decoder alone (the batch: the proposed end is
             * the stream's end, the frame's limit) */
            if (int rc = decode_frames_impl(ctx, d_data, bytes, q_off, 1, &p1, nullptr, (int32_t*)probe_rows.p, kProbeStride,
                                            (int32_t*)(q_off + 4), q_off + 3, q_off + 2, true, s, batch ? q_off + 1 : nullptr))
                return rc;
            HIP_TRY(hipMemcpyAsync(&k1s, q_off + 4, sizeof(k1s), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(&w.probe_end, q_off + 2, sizeof(int64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            w.probe_status = k1s;
            /* the proposed end was the chunk's: ending anywhere before it is no finding yet */
            if (!walk_ref_error(k1s) && (k1s >> 16) == FLACMI_DSITE_FRAME_END) w.probe_status = 0;
            ++sg.probes;
        }
        sg.nc = w.n_chain;
        sg.stop = w.state == FLACMI_WALK_STOPPED ? w.stop_status : 0;
        sg.pos = w.pos;
        for (int64_t i = 0; i < sg.nc; ++i)
            if (chain[(size_t)(total + i)].candidate >= 0) chain[(size_t)(total + i)].candidate += k0;
        total += sg.nc;
        h.probes += sg.probes;
    }

    /* block sizes; 5. pass 2: the chain frames whose pass-1 rows are not final, in runs of
     * neighbours, with the chain's own offsets */
    std::vector<int32_t>& bsz = h.bsz;
    std::vector<int64_t>& row2 = h.row2; /* index among the pass-2 frames */
    bsz.assign((size_t)total, 0);
    row2.assign((size_t)total, -1);
    int64_t n2 = 0, stride2 = 4;
    for (int64_t g = 0; g < nseg; ++g) {
        StreamFrames::Seg& sg = segs[(size_t)g];
        for (int64_t i = sg.c0; i < sg.c0 + sg.nc; ++i) {
            const flacmi_chain_frame& c = chain[i];
            if (c.candidate >= 0 && table[c.candidate].block_size > 0) {
                bsz[i] = table[c.candidate].block_size;
            } else {
                flacmi_frame_candidate h{};
                if (!parse_header(data, seg[g + 1], c.offset, false, h)) return fail(FLACMI_E_INVALID, "internal: chain frame without a header");
                bsz[i] = h.block_size;
            }
            if (c.status != 0) {
                row2[i] = n2++;
                ++sg.n2;
                stride2 = std::max<int64_t>(stride2, (bsz[i] + 3) & ~3);
            }
        }
    }
    h.n2 = n2;
    ScopedDev& rows2 = h.rows2;
    ScopedDev meta2;
    if (n2) {
        if (int rc = rows2.alloc(sizeof(int32_t) * (size_t)n2 * ch * (size_t)stride2)) return rc;
        if (int rc = meta2.alloc(40 * (size_t)n2 + 64)) return rc;
        /* offsets [2 n2] (a run of r frames uses r + 1), mismatch [n2], stream ends [n2] (the batch), status [n2] */
        int64_t* e_off = (int64_t*)meta2.p;
        int64_t* e_mm = e_off + 2 * n2;
        int64_t* e_lim = e_mm + n2;
        int32_t* e_st = (int32_t*)(e_lim + n2);
        std::vector<int64_t> off, lim2;
        std::vector<int32_t> st2((size_t)n2);
        struct Run { int64_t first2, count, off0; };
        std::vector<Run> runs;
        for (int64_t g = 0; g < nseg; ++g) { /* a run lies inside one stream */
            const int64_t c1 = segs[(size_t)g].c0 + segs[(size_t)g].nc;
            for (int64_t i = segs[(size_t)g].c0; i < c1;) {
                if (row2[i] < 0) { ++i; continue; }
                int64_t j = i;
                const int64_t o0 = (int64_t)off.size();
                while (j < c1 && row2[j] >= 0) off.push_back(chain[j++].offset);
                off.push_back(chain[j - 1].end);
                runs.push_back({row2[i], j - i, o0});
                lim2.insert(lim2.end(), (size_t)(j - i), seg[g + 1]);
                i = j;
            }
        }
        /* off holds n2 + (number of runs) <= 2 n2 entries */
        HIP_TRY(hipMemcpyAsync(e_off, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, s));
        if (batch) HIP_TRY(hipMemcpyAsync(e_lim, lim2.data(), sizeof(int64_t) * (size_t)n2, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (const Run& r : runs) {
            if (int rc = decode_frames_impl(ctx, d_data, bytes, e_off + r.off0, r.count, &p1, nullptr,
                                            (int32_t*)rows2.p + r.first2 * ch * stride2, stride2, e_st + r.first2, e_mm + r.first2,
                                            nullptr, false, s, batch ? e_lim + r.first2 : nullptr))
                return rc;
        }
        HIP_TRY(hipMemcpyAsync(st2.data(), e_st, sizeof(int32_t) * (size_t)n2, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int64_t g = 0; g < nseg; ++g) {
            StreamFrames::Seg& sg = segs[(size_t)g];
            for (int64_t i = sg.c0; i < sg.c0 + sg.nc; ++i) {
                if (row2[i] >= 0 && st2[row2[i]] != 0) { /* final: the stream stops at this frame */
                    sg.stop = st2[row2[i]];
                    sg.nc = i - sg.c0;
                    sg.pos = chain[i].offset;
                    break;
                }
            }
        }
    }

    h.nc = segs[0].nc; /* the single stream's */
    h.stop = segs[0].stop;
    h.pos = segs[0].pos;
    h.stride1 = stride1;
    h.stride2 = stride2;
    return 0;
}

int flacmi_decode_stream_host(flacmi_ctx* ctx, const uint8_t* data, int64_t bytes, int64_t first_byte,
                              const flacmi_decode_params* dp, int32_t max_block_size, int32_t final_chunk,
                              uint8_t* pcm, int64_t pcm_capacity, int32_t mode, int32_t bytes_per_sample,
                              flacmi_stream_result* res) {
    if (!ctx || !dp || !res) return fail(FLACMI_E_INVALID, "null argument");
    if (bytes < 0 || first_byte < 0 || first_byte > bytes || pcm_capacity < 0) return fail(FLACMI_E_INVALID, "bad size");
    if (bytes > 0 && !data) return fail(FLACMI_E_INVALID, "null buffer");
    if (pcm_capacity > 0 && !pcm) return fail(FLACMI_E_INVALID, "null pcm buffer");
    if (dp->channels < 1 || dp->channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (dp->sample_size < 4 || dp->sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 4..32");
    if (int rc = decode_flags_ok(dp)) return rc;
    if (max_block_size < 0 || max_block_size > FLACMI_MAX_BLOCK + 1) return fail(FLACMI_E_INVALID, "max_block_size must be 0..65536");
    if (mode != FLACMI_PCM_PACKED && mode != FLACMI_PCM_RAW32) return fail(FLACMI_E_INVALID, "mode must be a flacmi_pcm_mode");
    if (mode == FLACMI_PCM_PACKED && (bytes_per_sample < 1 || bytes_per_sample > 4))
        return fail(FLACMI_E_INVALID, "bytes_per_sample must be 1..4");
    memset(res, 0, sizeof(*res));
    res->consumed = first_byte;
    if (bytes == first_byte) return 0;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t s = ctx->stream;
    const int ch = dp->channels;
    const int B = mode == FLACMI_PCM_RAW32 ? 4 : bytes_per_sample;
    StreamFrames h;
    {
        const int rc = stream_frames(ctx, data, bytes, first_byte, dp, max_block_size, final_chunk, h);
        res->candidates = h.candidates;
        res->probes = h.probes;
        res->pass2_frames = h.n2;
        if (rc) return rc;
    }
    const std::vector<flacmi_chain_frame>& chain = h.chain;
    const std::vector<int32_t>& bsz = h.bsz;
    const std::vector<int64_t>& row2 = h.row2;
    const ScopedDev& rows2 = h.rows2;
    const int64_t stride1 = h.stride1, stride2 = h.stride2;
    int64_t nc = h.nc;
    int32_t stop = h.stop;
    struct { int64_t pos; } w{h.pos};

    /* 6. PCM: the frames that fit the caller's buffer */
    std::vector<flacmi_pcm_frame> pf((size_t)nc);
    int64_t first = 0;
    for (int64_t i = 0; i < nc; ++i) {
        if ((first + bsz[i]) * ch * B > pcm_capacity) { /* ends the call like a cut-off frame */
            if (i == 0) return fail(FLACMI_E_NOMEM, "pcm_capacity %lld holds no frame of %d samples", (long long)pcm_capacity, bsz[i]);
            nc = i;
            stop = 0;
            res->pcm_full = 1;
            w.pos = chain[i].offset;
            break;
        }
        const flacmi_chain_frame& c = chain[i];
        flacmi_pcm_frame& f = pf[i];
        if (row2[i] >= 0) {
            f.rows = (int32_t*)rows2.p + row2[i] * ch * stride2;
            f.stride = stride2;
        } else {
            f.rows = (int32_t*)ctx->sd_rows.p + c.candidate * ch * stride1;
            f.stride = stride1;
        }
        f.first_sample = first;
        f.block_size = bsz[i];
        f.reserved0 = 0;
        first += bsz[i];
    }
    if (nc > 0) {
        const int64_t total = first * ch * B;
        if (int rc = ensure_buf(ctx->sd_pcm, (size_t)total + 16)) return rc;
        ScopedDev d_pf;
        if (int rc = d_pf.alloc(sizeof(flacmi_pcm_frame) * (size_t)nc + 4 * (size_t)nc)) return rc;
        int32_t* d_ps = (int32_t*)((char*)d_pf.p + sizeof(flacmi_pcm_frame) * (size_t)nc);
        std::vector<int32_t> ps((size_t)nc);
        HIP_TRY(hipMemcpyAsync(d_pf.p, pf.data(), sizeof(flacmi_pcm_frame) * (size_t)nc, hipMemcpyHostToDevice, s));
        if (int rc = flacmi_pcm_out_device(ctx, (const flacmi_pcm_frame*)d_pf.p, nc, ch, B, mode, (uint8_t*)ctx->sd_pcm.p, total, d_ps, s))
            return rc;
        HIP_TRY(hipMemcpyAsync(ps.data(), d_ps, sizeof(int32_t) * (size_t)nc, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int64_t i = 0; i < nc; ++i) {
            if (ps[i] != 0) {
                stop = (ps[i] & 0xFFFF) == FLACMI_STATUS_OVERFLOW ? ((FLACMI_DSITE_PCM_RANGE << 16) | FLACMI_STATUS_OVERFLOW) : ps[i];
                nc = i;
                w.pos = chain[i].offset;
                first = pf[i].first_sample;
                break;
            }
        }
        /* 7. copy out */
        if (first > 0) HIP_TRY(hipMemcpy(pcm, ctx->sd_pcm.p, (size_t)(first * ch * B), hipMemcpyDeviceToHost));
    }
    res->frames = nc;
    res->samples = first;
    res->pcm_bytes = first * ch * B;
    res->consumed = w.pos;
    res->status = stop & 0xFFFF;
    res->site = (stop >> 16) & 0xFFFF;
    return 0;
}

/* ---- batch decoder -------------------------------------------------------------------- */
struct BatchState {
    bool valid = false;
    int32_t channels = 0, sample_size = 0;
    int64_t n_streams = 0, n_frames = 0;
    ScopedDev rows2;                    /* pass 2's rows (pass 1's are ctx->sd_rows) */
    DevBuf list, out;                   /* device: frames [n_frames], lengths [n_streams] i64, the same after a fetch's range
                                           findings, status [n_frames] i32; the host fetch's rows */
    std::vector<flacmi_pcm_frame> pf;   /* ordered by (stream, first_sample) */
    std::vector<int64_t> first;         /* [n_streams + 1]: stream s's frames are pf[first[s] .. first[s + 1]) */
    std::vector<int64_t> offset;        /* [n_frames]: the frame's byte offset in data */
    std::vector<flacmi_batch_stream_result> res;
};
static void batch_free(BatchState* bs) {
    if (!bs) return;
    if (bs->list.p) (void)hipFree(bs->list.p);
    if (bs->out.p) (void)hipFree(bs->out.p);
    delete bs;
}
static void batch_invalidate(flacmi_ctx* ctx) {
    if (ctx->batch) ctx->batch->valid = false;
}

int flacmi_decode_batch_host(flacmi_ctx* ctx, const uint8_t* data, const int64_t* seg_offsets, int64_t n_streams,
                             const flacmi_decode_params* dp, int32_t max_block_size, flacmi_batch_stream_result* results,
                             flacmi_batch_summary* summary) {
    if (!dp || !results || !summary || !seg_offsets) return fail(FLACMI_E_INVALID, "null argument");
    if (n_streams < 1) return fail(FLACMI_E_INVALID, "n_streams must be at least 1");
    if (seg_offsets[0] != 0) return fail(FLACMI_E_INVALID, "seg_offsets must start at 0");
    for (int64_t g = 0; g < n_streams; ++g)
        if (seg_offsets[g + 1] < seg_offsets[g]) return fail(FLACMI_E_INVALID, "seg_offsets descend at stream %lld", (long long)g);
    if (n_streams > 0x7FFFFFFF) return fail(FLACMI_E_UNSUPPORTED, "more than 2^31 - 1 streams in one call");
    const int64_t bytes = seg_offsets[n_streams];
    if (bytes > 0 && !data) return fail(FLACMI_E_INVALID, "null buffer");
    if (dp->channels < 1 || dp->channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (dp->sample_size < 4 || dp->sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 4..32");
    if (int rc = decode_flags_ok(dp)) return rc;
    if (max_block_size < 0 || max_block_size > FLACMI_MAX_BLOCK + 1) return fail(FLACMI_E_INVALID, "max_block_size must be 0..65536");
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    memset(results, 0, sizeof(*results) * (size_t)n_streams);
    memset(summary, 0, sizeof(*summary));
    for (int64_t g = 0; g < n_streams; ++g) results[g].consumed = seg_offsets[g];
    if (int rc = set_device(ctx)) return rc;
    if (!ctx->batch) ctx->batch = new BatchState();
    BatchState& b = *ctx->batch;
    b.valid = false;
    b.channels = dp->channels;
    b.sample_size = dp->sample_size;
    b.n_streams = n_streams;
    b.n_frames = 0;
    b.pf.clear();
    b.offset.clear();
    b.first.assign((size_t)n_streams + 1, 0);
    b.res.assign(results, results + n_streams);
    if (b.rows2.p) {
        HIP_TRY(hipFree(b.rows2.p));
        b.rows2.p = nullptr;
    }
    const int ch = dp->channels;
    if (bytes > 0) {
        StreamFrames h;
        const int rc = stream_frames(ctx, data, bytes, 0, dp, max_block_size, 1, h, seg_offsets, n_streams);
        summary->candidates = h.candidates;
        summary->probes = h.probes;
        summary->pass2_frames = h.n2;
        if (rc) return rc;
        std::swap(b.rows2.p, h.rows2.p);
        for (int64_t g = 0; g < n_streams; ++g) {
            const StreamFrames::Seg& sg = h.segs[(size_t)g];
            flacmi_batch_stream_result& r = b.res[(size_t)g];
            int64_t first = 0;
            b.first[(size_t)g] = (int64_t)b.pf.size();
            for (int64_t i = sg.c0; i < sg.c0 + sg.nc; ++i) {
                flacmi_pcm_frame f{};
                if (h.row2[i] >= 0) {
                    f.rows = (int32_t*)b.rows2.p + h.row2[i] * ch * h.stride2;
                    f.stride = h.stride2;
                } else {
                    f.rows = (int32_t*)ctx->sd_rows.p + h.chain[i].candidate * ch * h.stride1;
                    f.stride = h.stride1;
                }
                f.first_sample = first;
                f.block_size = h.bsz[i];
                f.reserved0 = (int32_t)g;
                first += h.bsz[i];
                b.pf.push_back(f);
                b.offset.push_back(h.chain[i].offset);
            }
            r.frames = sg.nc;
            r.samples = first;
            r.consumed = sg.pos;
            r.status = sg.stop & 0xFFFF;
            r.site = (sg.stop >> 16) & 0xFFFF;
            r.probes = sg.probes;
            r.pass2_frames = sg.n2;
        }
    }
    b.first[(size_t)n_streams] = (int64_t)b.pf.size();
    b.n_frames = (int64_t)b.pf.size();
    /* the list on the device, with the streams' lengths and room for the status words */
    const size_t nf = (size_t)b.n_frames;
    if (int rc = ensure_buf(b.list, (sizeof(flacmi_pcm_frame) + 4) * nf + 16 * (size_t)n_streams + 16)) return rc;
    hipStream_t s = ctx->stream;
    if (nf) HIP_TRY(hipMemcpyAsync(b.list.p, b.pf.data(), sizeof(flacmi_pcm_frame) * nf, hipMemcpyHostToDevice, s));
    std::vector<int64_t> len((size_t)n_streams);
    for (int64_t g = 0; g < n_streams; ++g) {
        len[(size_t)g] = b.res[(size_t)g].samples;
        summary->frames += b.res[(size_t)g].frames;
        summary->max_samples = std::max(summary->max_samples, b.res[(size_t)g].samples);
    }
    HIP_TRY(hipMemcpyAsync((char*)b.list.p + sizeof(flacmi_pcm_frame) * nf, len.data(), 8 * (size_t)n_streams, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(results, b.res.data(), sizeof(*results) * (size_t)n_streams);
    b.valid = true;
    return 0;
}

int flacmi_decode_batch_fetch(flacmi_ctx* ctx, void* out, int64_t pitch, int32_t elem, int32_t host_out,
                              flacmi_batch_stream_result* results, void* stream) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (!ctx->batch || !ctx->batch->valid)
        return fail(FLACMI_E_INVALID, "no frame list: flacmi_decode_batch_host must be the context's last decode call");
    BatchState& b = *ctx->batch;
    if (elem != FLACMI_PLANAR_INT16 && elem != FLACMI_PLANAR_INT32 && elem != FLACMI_PLANAR_FLOAT32)
        return fail(FLACMI_E_INVALID, "elem must be a flacmi_planar_elem");
    const int sb = elem == FLACMI_PLANAR_INT16 ? 2 : 4;
    int64_t longest = 0;
    for (const auto& r : b.res) longest = std::max(longest, r.samples);
    if (pitch < longest || (pitch * sb) % 16 != 0)
        return fail(FLACMI_E_INVALID, "pitch must hold %lld samples and be a multiple of 16 bytes", (long long)longest);
    if (pitch > 0 && !out) return fail(FLACMI_E_INVALID, "null out");
    if (int rc = set_device(ctx)) return rc;
    hipStream_t s = host_out ? ctx->stream : (hipStream_t)stream;
    const size_t nf = (size_t)b.n_frames, total = (size_t)b.n_streams * b.channels * (size_t)pitch * sb;
    void* d_out = out;
    if (host_out) {
        if (int rc = ensure_buf(b.out, total + 16)) return rc;
        d_out = b.out.p;
    }
    const flacmi_pcm_frame* d_pf = (const flacmi_pcm_frame*)b.list.p;
    int64_t* d_len = (int64_t*)((char*)b.list.p + sizeof(flacmi_pcm_frame) * nf);
    int64_t* d_cut = d_len + b.n_streams;
    int32_t* d_st = (int32_t*)(d_cut + b.n_streams);
    std::vector<flacmi_batch_stream_result> res = b.res; /* the list stays whole for a later fetch of another type */
    if (int rc = flacmi_planar_out_device(ctx, d_pf, b.n_frames, b.n_streams, b.channels, d_len, b.sample_size, elem, d_out, pitch,
                                          d_st, s))
        return rc;
    if (elem == FLACMI_PLANAR_INT16 && nf > 0) { /* a range finding stops its stream at that frame */
        std::vector<int32_t> st(nf);
        HIP_TRY(hipMemcpyAsync(st.data(), d_st, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        bool again = false;
        std::vector<int64_t> len((size_t)b.n_streams);
        for (int64_t g = 0; g < b.n_streams; ++g) {
            flacmi_batch_stream_result& r = res[(size_t)g];
            for (int64_t i = b.first[(size_t)g]; i < b.first[(size_t)g] + r.frames; ++i) {
                if (st[(size_t)i] == 0) continue;
                r.frames = i - b.first[(size_t)g];
                r.samples = b.pf[(size_t)i].first_sample;
                r.consumed = b.offset[(size_t)i];
                r.status = FLACMI_STATUS_OVERFLOW;
                r.site = FLACMI_DSITE_PCM_RANGE;
                again = true;
                break;
            }
            len[(size_t)g] = r.samples;
        }
        if (again) { /* rare: the rows again, cut at the final lengths */
            HIP_TRY(hipMemcpyAsync(d_cut, len.data(), 8 * (size_t)b.n_streams, hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s)); /* len is a local */
            if (int rc = flacmi_planar_out_device(ctx, d_pf, b.n_frames, b.n_streams, b.channels, d_cut, b.sample_size, elem, d_out,
                                                  pitch, d_st, s))
                return rc;
        }
    }
    if (host_out && total > 0) {
        HIP_TRY(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (results) memcpy(results, res.data(), sizeof(*results) * (size_t)b.n_streams);
    return 0;
}

/* ---- stream analysis ------------------------------------------------------------------- */
int flacmi_frame_info_device(flacmi_ctx* ctx, const uint8_t* stream_data, int64_t stream_bytes,
                             const int64_t* frame_offsets, int64_t n_frames, const flacmi_decode_params* dp,
                             flacmi_frame_info* frame_info, flacmi_subframe_info* subframe_info,
                             uint8_t* part_params, int64_t part_stride, void* stream) {
    if (!ctx || !dp) return fail(FLACMI_E_INVALID, "null argument");
    if (n_frames < 0 || stream_bytes < 0) return fail(FLACMI_E_INVALID, "negative size");
    if (part_stride < 0 || part_stride > 32768) return fail(FLACMI_E_INVALID, "part_stride must be 0..32768");
    if (n_frames == 0) return 0;
    if (!stream_data || !frame_offsets || !frame_info || !subframe_info) return fail(FLACMI_E_INVALID, "null buffer");
    if (part_stride > 0 && !part_params) return fail(FLACMI_E_INVALID, "null part_params");
    if (((uintptr_t)stream_data & 3) != 0) return fail(FLACMI_E_INVALID, "stream_data must be 4-byte aligned");
    if ((((uintptr_t)frame_info | (uintptr_t)subframe_info | (uintptr_t)frame_offsets) & 7) != 0)
        return fail(FLACMI_E_INVALID, "frame_offsets, frame_info and subframe_info must be 8-byte aligned");
    if (dp->channels < 1 || dp->channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (dp->sample_size < 4 || dp->sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 4..32");
    if (int rc = decode_flags_ok(dp)) return rc;
    if (int rc = set_device(ctx)) return rc;
    InfoArgs a{};
    a.words = reinterpret_cast<const uint32_t*>(stream_data);
    a.stream_bytes = stream_bytes;
    a.n_words = (stream_bytes + 3) / 4;
    a.offsets = frame_offsets;
    a.n_frames = n_frames;
    a.channels = dp->channels;
    a.sample_size = dp->sample_size;
    a.frames = frame_info;
    a.subs = subframe_info;
    a.parts = part_stride > 0 ? part_params : nullptr;
    a.part_stride = (int32_t)part_stride;
    a.crc_slice = ctx->d_crc;
    a.wasted_spec = (dp->reserved0 & FLACMI_DECODE_WASTED_SPEC) != 0;
    HIP_TRY(launch_frame_info(a, knob(kKnobInfoGrid), (hipStream_t)stream));
    return 0;
}

int flacmi_info_stream_host(flacmi_ctx* ctx, const uint8_t* data, int64_t bytes, int64_t first_byte,
                            const flacmi_decode_params* dp, int32_t final_chunk, flacmi_frame_info* frame_info,
                            flacmi_subframe_info* subframe_info, uint8_t* part_params, int64_t part_stride,
                            int64_t frame_capacity, flacmi_info_result* res) {
    if (!ctx || !dp || !res) return fail(FLACMI_E_INVALID, "null argument");
    if (bytes < 0 || first_byte < 0 || first_byte > bytes || frame_capacity < 0) return fail(FLACMI_E_INVALID, "bad size");
    if (bytes > 0 && !data) return fail(FLACMI_E_INVALID, "null buffer");
    if (frame_capacity > 0 && (!frame_info || !subframe_info)) return fail(FLACMI_E_INVALID, "null record buffer");
    if (part_stride < 0 || part_stride > 32768) return fail(FLACMI_E_INVALID, "part_stride must be 0..32768");
    if (part_stride > 0 && frame_capacity > 0 && !part_params) return fail(FLACMI_E_INVALID, "null part_params");
    if (dp->channels < 1 || dp->channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (dp->sample_size < 4 || dp->sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 4..32");
    if (int rc = decode_flags_ok(dp)) return rc;
    memset(res, 0, sizeof(*res));
    res->consumed = first_byte;
    if (bytes == first_byte) return 0;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t s = ctx->stream;
    const size_t ch = (size_t)dp->channels, ps = (size_t)part_stride;

    /* 1. the chunk, 2. the index (as flacmi_decode_stream_host) */
    if (int rc = ensure_buf(ctx->sd_data, (size_t)bytes + 32)) return rc;
    uint8_t* d_data = (uint8_t*)ctx->sd_data.p;
    HIP_TRY(hipMemcpyAsync(d_data, data, (size_t)bytes, hipMemcpyHostToDevice, s));
    int64_t cap = bytes / 512 + 1024, n = 0;
    for (;;) {
        if (int rc = ensure_buf(ctx->sd_table, sizeof(flacmi_frame_candidate) * (size_t)cap + 16)) return rc;
        int64_t* d_count = (int64_t*)ctx->sd_table.p;
        if (int rc = flacmi_index_frames_device(ctx, d_data, bytes, first_byte,
                                                (flacmi_frame_candidate*)((char*)ctx->sd_table.p + 16), cap, d_count, s))
            return rc;
        HIP_TRY(hipMemcpyAsync(&n, d_count, sizeof(n), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n <= cap) break;
        cap = n;
    }
    res->candidates = n;
    std::vector<flacmi_frame_candidate> table((size_t)n);
    if (n) HIP_TRY(hipMemcpy(table.data(), (char*)ctx->sd_table.p + 16, sizeof(flacmi_frame_candidate) * (size_t)n, hipMemcpyDeviceToHost));

    /* 3. k_frame_info over every candidate (slot n: the probes'), 4. the records out */
    const size_t slots = (size_t)n + 1;
    if (int rc = ensure_buf(ctx->sd_meta, sizeof(int64_t) * slots + 64)) return rc;
    if (int rc = ensure_buf(ctx->si_frames, sizeof(flacmi_frame_info) * slots)) return rc;
    if (int rc = ensure_buf(ctx->si_subs, sizeof(flacmi_subframe_info) * slots * ch)) return rc;
    if (int rc = ensure_buf(ctx->si_parts, slots * ch * ps + 16)) return rc;
    int64_t* d_off = (int64_t*)ctx->sd_meta.p;
    flacmi_frame_info* d_fi = (flacmi_frame_info*)ctx->si_frames.p;
    flacmi_subframe_info* d_si = (flacmi_subframe_info*)ctx->si_subs.p;
    uint8_t* d_pp = (uint8_t*)ctx->si_parts.p;
    std::vector<flacmi_frame_info> fi((size_t)n);
    std::vector<flacmi_subframe_info> si((size_t)n * ch);
    std::vector<uint8_t> pp((size_t)n * ch * ps);
    std::vector<int32_t> st1((size_t)n);
    std::vector<int64_t> end1((size_t)n);
    /* a parsed frame's end is its own, not the next candidate's offset: a word that is no
     * reference exception makes the walk read frame_end */
    constexpr int32_t kParsed = (FLACMI_DSITE_FRAME_END << 16) | FLACMI_STATUS_VERIFY;
    if (n) {
        std::vector<int64_t> off((size_t)n);
        for (int64_t k = 0; k < n; ++k) off[k] = table[k].offset;
        HIP_TRY(hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
        if (int rc = flacmi_frame_info_device(ctx, d_data, bytes, d_off, n, dp, d_fi, d_si, d_pp, part_stride, s)) return rc;
        HIP_TRY(hipMemcpyAsync(fi.data(), d_fi, sizeof(flacmi_frame_info) * (size_t)n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(si.data(), d_si, sizeof(flacmi_subframe_info) * (size_t)n * ch, hipMemcpyDeviceToHost, s));
        if (!pp.empty()) HIP_TRY(hipMemcpyAsync(pp.data(), d_pp, pp.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s)); /* off is a local vector */
        for (int64_t k = 0; k < n; ++k) {
            st1[k] = fi[k].status ? fi[k].status : kParsed;
            end1[k] = fi[k].end;
        }
    }

    /* 5. the walk; a probe parses the one frame at w.pos into slot n */
    struct Probed {
        flacmi_frame_info fi;
        std::vector<flacmi_subframe_info> si;
        std::vector<uint8_t> pp;
    };
    std::map<int64_t, Probed> probed; /* by offset */
    std::vector<flacmi_chain_frame> chain((size_t)n + 16);
    flacmi_walk w{};
    w.pos = first_byte;
    for (;;) {
        if (int rc = flacmi_host_chain_walk(table.data(), n, st1.data(), end1.data(), bytes, final_chunk, &w, chain.data(),
                                            (int64_t)chain.size()))
            return rc;
        if (w.state == FLACMI_WALK_FULL) {
            chain.resize(chain.size() * 2);
            w.state = FLACMI_WALK_RUN;
            continue;
        }
        if (w.state != FLACMI_WALK_PROBE) break;
        if ((int64_t)chain.size() == w.n_chain) chain.resize(chain.size() * 2);
        Probed& q = probed[w.pos];
        q.si.resize(ch);
        q.pp.resize(ch * ps);
        const int64_t at = w.pos;
        HIP_TRY(hipMemcpyAsync(d_off + n, &at, sizeof(at), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); /* `at` is a local */
        if (int rc = flacmi_frame_info_device(ctx, d_data, bytes, d_off + n, 1, dp, d_fi + n, d_si + (size_t)n * ch,
                                              d_pp + (size_t)n * ch * ps, part_stride, s))
            return rc;
        HIP_TRY(hipMemcpyAsync(&q.fi, d_fi + n, sizeof(flacmi_frame_info), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(q.si.data(), d_si + (size_t)n * ch, sizeof(flacmi_subframe_info) * ch, hipMemcpyDeviceToHost, s));
        if (!q.pp.empty()) HIP_TRY(hipMemcpyAsync(q.pp.data(), d_pp + (size_t)n * ch * ps, q.pp.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        w.probe_status = q.fi.status;
        w.probe_end = q.fi.end;
        ++res->probes;
    }
    int64_t nc = w.n_chain;
    int32_t stop = w.state == FLACMI_WALK_STOPPED ? w.stop_status : 0;
    if (nc > frame_capacity) { /* ends the call like a cut-off frame */
        nc = frame_capacity;
        stop = 0;
        res->full = 1;
        w.pos = chain[nc].offset;
    }

    /* 6. the chain frames' records, in stream order */
    for (int64_t i = 0; i < nc; ++i) {
        const flacmi_chain_frame& c = chain[i];
        const flacmi_frame_info* f1;
        const flacmi_subframe_info* s1;
        const uint8_t* p1;
        if (c.candidate >= 0) {
            f1 = &fi[c.candidate];
            s1 = si.data() + (size_t)c.candidate * ch;
            p1 = pp.data() + (size_t)c.candidate * ch * ps;
        } else {
            auto it = probed.find(c.offset);
            if (it == probed.end()) return fail(FLACMI_E_INVALID, "internal: chain frame without a record");
            f1 = &it->second.fi;
            s1 = it->second.si.data();
            p1 = it->second.pp.data();
        }
        frame_info[i] = *f1;
        memcpy(subframe_info + (size_t)i * ch, s1, sizeof(flacmi_subframe_info) * ch);
        if (ps) memcpy(part_params + (size_t)i * ch * ps, p1, ch * ps);
    }
    res->frames = nc;
    res->consumed = w.pos;
    res->status = stop & 0xFFFF;
    res->site = (stop >> 16) & 0xFFFF;
    return 0;
}

/* The context buffers encode_rows writes (everything but the sample rows, which its caller fills) */
static int encode_rows_buffers(flacmi_ctx* ctx, size_t nu, int64_t nf, const flacmi_params* params,
                               const flacmi_frame_params* fp) {
    const size_t nou = stereo_out_units(fp, nu); /* units of the analysis outputs */
    const int64_t pstride = (1LL << (params->rice_max > 0 ? params->rice_max : 0)) + 1;
    if (int rc = ensure_buf(ctx->h_meta, nou * sizeof(flacmi_unit_meta))) return rc;
    if (int rc = ensure_buf(ctx->h_params, nou * pstride * sizeof(int32_t))) return rc;
    if (int rc = ensure_buf(ctx->h_offsets, sizeof(int64_t) * (size_t)(nf + 1))) return rc;
    if (int rc = ensure_buf(ctx->h_status, sizeof(int32_t) * (size_t)nf)) return rc;
    return 0;
}

/* flacmi_encode_host behind its copy in, shared with flacmi_recompress_host: db is a device batch
 * in ctx->h_samples (in the stereo mode with room for the mid rows behind it) that this call may
 * shift in place (the wasted-bits mode, once per copy of the rows); params already went through
 * size_choice_params.  The frames stay in ctx->h_frames, frame_offsets / frame_status are host
 * arrays. */
static int encode_rows(flacmi_ctx* ctx, const flacmi_batch& db, const flacmi_params* params,
                       const flacmi_frame_params* fp, int64_t nf, int64_t* frame_offsets, int32_t* frame_status) {
    const flacmi_batch* batch = &db;
    const size_t nu = (size_t)db.n_units;
    const bool stereo = stereo_on(fp);
    const size_t nou = stereo_out_units(fp, nu);
    const int64_t pstride = (1LL << (params->rice_max > 0 ? params->rice_max : 0)) + 1;
    if (int rc = wasted_shift(fp, db, ctx->h_wasted, ctx->stream)) return rc; /* once, before the redo loop */
    for (int rbytes = 4;; rbytes = 8) {
        const int64_t rstride = ((batch->block_len * rbytes + 15) / 16) * 16 / rbytes;
        if (int rc = ensure_buf(ctx->h_residual, nou * rstride * rbytes)) return rc;
        flacmi_outputs o{};
        o.meta = (flacmi_unit_meta*)ctx->h_meta.p;
        o.rice_params = (int32_t*)ctx->h_params.p;
        o.params_stride = pstride;
        o.residual = ctx->h_residual.p;
        o.residual_bytes = rbytes;
        o.residual_stride = rstride;
        if (stereo) {
            if (int rc = stereo_analyze(ctx, db, params, o, ctx->h_side, ctx->stream, true)) return rc;
        } else {
            if (int rc = validate(&db, params, &o)) return rc;
            if (int rc = analyze_device_impl(ctx, &db, params, &o, ctx->stream)) return rc;
        }
        FrameArgs a = frame_args(ctx, &db, fp, o.meta, o.rice_params, pstride, nf);
        if (int rc = stereo_args(fp, db, ctx->h_side, ctx->h_choice, a)) return rc;
        if (int rc = own_sub_kind(fp, ctx->h_subkind, a)) return rc;
        wasted_args(fp, ctx->h_wasted, a);
        if (int rc = frame_sizes_impl(ctx, a, (int64_t*)ctx->h_offsets.p, (int32_t*)ctx->h_status.p, ctx->stream))
            return rc;
        HIP_TRY(hipMemcpyAsync(frame_offsets, ctx->h_offsets.p, sizeof(int64_t) * (nf + 1), hipMemcpyDeviceToHost,
                               ctx->stream));
        HIP_TRY(hipMemcpyAsync(frame_status, ctx->h_status.p, sizeof(int32_t) * nf, hipMemcpyDeviceToHost,
                               ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        bool wide = false;
        for (int64_t f = 0; f < nf && rbytes == 4; ++f)
            if ((frame_status[f] & 0xffff) == FLACMI_STATUS_RESIDUAL_WIDE) wide = true;
        if (wide) continue; /* a chosen residual needs 64 bits: redo with 8-byte rows */
        const int64_t total = frame_offsets[nf];
        if (int rc = ensure_buf(ctx->h_frames, (size_t)total + 16)) return rc;
        a.residual = ctx->h_residual.p;
        a.residual_bytes = rbytes;
        a.residual_stride = rstride;
        a.offsets = (int64_t*)ctx->h_offsets.p;
        a.status = (int32_t*)ctx->h_status.p;
        a.out = (uint8_t*)ctx->h_frames.p;
        a.capacity = total;
        if (int rc = pack_lists(ctx, a)) return rc;
        HIP_TRY(launch_pack(a, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->frames_bytes = total;
        return 0;
    }
}

int flacmi_encode_host(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_params* params,
                       const flacmi_frame_params* fp, int64_t* frame_offsets, int32_t* frame_status) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    int64_t nf = 0;
    if (int rc = validate_frames(batch, fp, &nf)) return rc;
    if (!params || !frame_offsets || !frame_status) return fail(FLACMI_E_INVALID, "null argument");
    flacmi_params sized;
    if (int rc = size_choice_params(params, fp, &sized)) return rc;
    params = &sized;
    ctx->frames_bytes = 0;
    if (nf == 0) {
        frame_offsets[0] = 0;
        return 0;
    }
    if (int rc = set_device(ctx)) return rc;
    const size_t nu = (size_t)batch->n_units;
    const int64_t sstride = row_pitch(batch->block_len, batch->sample_bytes);
    if (int rc = ensure_buf(ctx->h_samples, stereo_sample_rows(fp, nu) * sstride * batch->sample_bytes)) return rc;
    if (int rc = encode_rows_buffers(ctx, nu, nf, params, fp)) return rc;
    flacmi_batch db = *batch;
    db.samples = ctx->h_samples.p;
    db.unit_stride = sstride;
    HIP_TRY(hipMemcpy2DAsync(ctx->h_samples.p, sstride * batch->sample_bytes, batch->samples,
                             batch->unit_stride * batch->sample_bytes, batch->block_len * batch->sample_bytes, nu,
                             hipMemcpyHostToDevice, ctx->stream));
    return encode_rows(ctx, db, params, fp, nf, frame_offsets, frame_status);
}

/* ---- recompress: stream_frames, k_units, encode_rows -------------------------------------
 * The frame list of a call is the carry (a pseudo-frame at sample 0 over the current carry
 * buffer) followed by the chain's frames.  The first k_units launch cuts it into the call's unit
 * rows (ctx->h_samples, where flacmi_encode_host keeps its copy of the rows), the second writes
 * the samples behind the last whole block into the other carry buffer, so each sample is
 * range-checked by the call that decoded it.  A range finding in frame j stops the input there:
 * the blocks entirely before j's first sample hold none of its samples and are already written. */
int flacmi_recompress_host(flacmi_ctx* ctx, const uint8_t* data, int64_t bytes, int64_t first_byte,
                           const flacmi_decode_params* dp, int32_t max_block_size, int32_t final_chunk,
                           int32_t restart, int32_t block_len, const flacmi_params* params,
                           const flacmi_frame_params* fp, flacmi_recompress_result* res) {
    if (!ctx || !dp || !res || !params || !fp) return fail(FLACMI_E_INVALID, "null argument");
    if (bytes < 0 || first_byte < 0 || first_byte > bytes) return fail(FLACMI_E_INVALID, "bad size");
    if (bytes > 0 && !data) return fail(FLACMI_E_INVALID, "null buffer");
    if (dp->channels < 1 || dp->channels > 8) return fail(FLACMI_E_INVALID, "channels must be 1..8");
    if (dp->sample_size < 4 || dp->sample_size > 32) return fail(FLACMI_E_INVALID, "sample_size must be 4..32");
    if (int rc = decode_flags_ok(dp)) return rc;
    if (max_block_size < 0 || max_block_size > FLACMI_MAX_BLOCK + 1) return fail(FLACMI_E_INVALID, "max_block_size must be 0..65536");
    if (block_len < 1 || block_len > FLACMI_MAX_BLOCK) return fail(FLACMI_E_INVALID, "block_len must be 1..65535");
    /* whatever flacmi_encode_host refuses for these params / fp, on a batch of this shape */
    const int sbytes = fp->sample_size <= 16 ? 2 : 4;
    const int64_t sstride = row_pitch(block_len, sbytes);
    flacmi_batch vb{};
    vb.samples = (const void*)(uintptr_t)16;
    vb.sample_bytes = sbytes;
    vb.sample_bits = 2;
    vb.unit_stride = sstride;
    vb.block_len = block_len;
    int64_t nf = 0;
    if (int rc = validate_frames(&vb, fp, &nf)) return rc;
    flacmi_params sized;
    if (int rc = size_choice_params(params, fp, &sized)) return rc;
    if (dp->channels != fp->channels || dp->sample_size != fp->sample_size)
        return fail(FLACMI_E_INVALID, "dp and fp disagree on channels or sample_size");
    {
        flacmi_outputs vo{};
        vo.meta = (flacmi_unit_meta*)(uintptr_t)16;
        vo.rice_params = (int32_t*)(uintptr_t)16;
        vo.residual = (void*)(uintptr_t)16;
        vo.residual_bytes = 4;
        vo.residual_stride = ((block_len * 4 + 15) / 16) * 16 / 4;
        vo.params_stride = (1LL << (sized.rice_max > 0 ? sized.rice_max : 0)) + 1;
        if (int rc = validate(&vb, &sized, &vo)) return rc;
    }
    const int ch = fp->channels, B = block_len;
    memset(res, 0, sizeof(*res));
    res->consumed = first_byte;
    ctx->frames_bytes = 0;
    ctx->rc_offsets.assign(1, 0);
    ctx->rc_status.clear();
    if (restart) {
        ctx->rc_carry_len = 0;
        ctx->rc_blocks = 0;
    }
    if (ctx->rc_carry_len > 0 && ctx->rc_channels != ch)
        return fail(FLACMI_E_INVALID, "the carry holds %d channels, the call has %d: restart first", ctx->rc_channels, ch);
    res->carry = ctx->rc_carry_len;
    if (bytes == first_byte && !(final_chunk && ctx->rc_carry_len > 0)) return 0;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t s = ctx->stream;

    StreamFrames h;
    h.pos = first_byte;
    if (bytes > first_byte) {
        const int rc = stream_frames(ctx, data, bytes, first_byte, dp, max_block_size, final_chunk, h);
        res->candidates = h.candidates;
        res->probes = h.probes;
        res->pass2_frames = h.n2;
        if (rc) return rc;
    }
    int64_t nc = h.nc, pos = h.pos;
    int32_t stop = h.stop;
    const bool at_end = final_chunk && stop == 0;
    const int32_t carry_in = ctx->rc_carry_len;
    if (nc == 0 && stop == 0 && !at_end) return 0; /* no whole frame in the chunk: the carry stays */

    /* the frame list */
    const int64_t nl = nc + 1;
    std::vector<flacmi_pcm_frame> pf((size_t)nl);
    pf[0] = flacmi_pcm_frame{ctx->rc_carry[ctx->rc_cur].p, ctx->rc_stride[ctx->rc_cur], 0, carry_in, 0};
    int64_t total = carry_in;
    for (int64_t i = 0; i < nc; ++i) {
        flacmi_pcm_frame& f = pf[(size_t)i + 1];
        if (h.row2[i] >= 0) {
            f.rows = (int32_t*)h.rows2.p + h.row2[i] * ch * h.stride2;
            f.stride = h.stride2;
        } else {
            f.rows = (int32_t*)ctx->sd_rows.p + h.chain[i].candidate * ch * h.stride1;
            f.stride = h.stride1;
        }
        f.first_sample = total;
        f.block_size = h.bsz[i];
        f.reserved0 = 0;
        total += h.bsz[i];
    }
    int64_t n_blocks = total / B;
    int32_t tail = at_end ? (int32_t)(total % B) : 0;
    /* the samples behind the last whole block: range-checked even where a later frame's status drops them */
    const int32_t rest = at_end ? 0 : (int32_t)(total % B);
    int32_t left = stop == 0 ? rest : 0;

    /* device words behind the list: status of the first launch [nl], of the second [nl], the two widths */
    if (int rc = ensure_buf(ctx->rc_list, (sizeof(flacmi_pcm_frame) + 8) * (size_t)nl + 16)) return rc;
    flacmi_pcm_frame* d_pf = (flacmi_pcm_frame*)ctx->rc_list.p;
    int32_t* d_st1 = (int32_t*)(d_pf + nl);
    int32_t* d_st2 = d_st1 + nl;
    uint32_t* d_w = (uint32_t*)(d_st2 + nl);
    HIP_TRY(hipMemcpyAsync(d_pf, pf.data(), sizeof(flacmi_pcm_frame) * (size_t)nl, hipMemcpyHostToDevice, s));
    const size_t nu0 = (size_t)(n_blocks + (tail > 0 ? 1 : 0)) * ch;
    if (nu0 > 0)
        if (int rc = ensure_buf(ctx->h_samples, stereo_sample_rows(fp, nu0) * sstride * sbytes)) return rc;
    if (int rc = flacmi_units_out_device(ctx, d_pf, nl, ch, 0, B, n_blocks, tail, fp->sample_size, ctx->h_samples.p, sbytes,
                                         sstride, d_st1, d_w, s))
        return rc;
    std::vector<int32_t> st((size_t)(2 * nl), 0);
    const int other = ctx->rc_cur ^ 1;
    if (rest > 0) {
        const int64_t cstride = row_pitch(B, 4);
        if (int rc = ensure_buf(ctx->rc_carry[other], sizeof(int32_t) * (size_t)ch * cstride)) return rc;
        ctx->rc_stride[other] = cstride;
        if (int rc = flacmi_units_out_device(ctx, d_pf, nl, ch, n_blocks * B, B, 0, rest, fp->sample_size,
                                             ctx->rc_carry[other].p, 4, cstride, d_st2, d_w + 1, s))
            return rc;
    }
    uint32_t width = 0;
    HIP_TRY(hipMemcpyAsync(st.data(), d_st1, sizeof(int32_t) * (size_t)(rest > 0 ? 2 * nl : nl), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&width, d_w, sizeof(width), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t j = 0; j < nl; ++j) {
        if ((st[j] | st[nl + j]) == 0) continue;
        stop = (FLACMI_DSITE_PCM_RANGE << 16) | FLACMI_STATUS_OVERFLOW;
        nc = j > 0 ? j - 1 : 0;
        pos = j > 0 ? h.chain[j - 1].offset : first_byte;
        total = pf[j].first_sample;
        n_blocks = total / B;
        tail = 0;
        left = 0;
        break;
    }

    /* the encode half over the blocks that stand */
    nf = n_blocks + (tail > 0 ? 1 : 0);
    if (nf > 0) {
        int bl = 0;
        while (bl < 32 && (width >> bl) != 0) ++bl;
        flacmi_batch db{};
        db.samples = ctx->h_samples.p;
        db.sample_bytes = sbytes;
        db.sample_bits = std::min<int>(fp->sample_size, std::max(2, bl + 1));
        db.unit_stride = sstride;
        db.n_units = nf * ch;
        db.block_len = B;
        db.tail_len = tail;
        db.n_tail_units = tail > 0 ? ch : 0;
        flacmi_frame_params f2 = *fp;
        f2.first_frame = fp->first_frame + ctx->rc_blocks;
        ctx->rc_offsets.assign((size_t)nf + 1, 0);
        ctx->rc_status.assign((size_t)nf, 0);
        if (int rc = encode_rows_buffers(ctx, (size_t)db.n_units, nf, &sized, &f2)) return rc;
        if (int rc = encode_rows(ctx, db, &sized, &f2, nf, ctx->rc_offsets.data(), ctx->rc_status.data())) return rc;
        ctx->rc_blocks += nf;
        res->sample_bits = db.sample_bits;
    }
    if (left > 0) {
        ctx->rc_cur = other;
        ctx->rc_channels = ch;
    }
    ctx->rc_carry_len = left;
    res->frames = nc;
    res->samples = nc > 0 ? pf[(size_t)nc].first_sample + pf[(size_t)nc].block_size - carry_in : 0;
    res->consumed = pos;
    res->status = stop & 0xFFFF;
    res->site = (stop >> 16) & 0xFFFF;
    res->blocks_out = nf;
    res->frame_bytes = ctx->frames_bytes;
    res->carry = left;
    return 0;
}

int flacmi_recompress_fetch(flacmi_ctx* ctx, int64_t* frame_offsets, int32_t* frame_status, int64_t n_blocks,
                            uint8_t* out, int64_t bytes) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (n_blocks != (int64_t)ctx->rc_status.size())
        return fail(FLACMI_E_INVALID, "the last flacmi_recompress_host call wrote %zu blocks", ctx->rc_status.size());
    if (!frame_offsets || (n_blocks > 0 && !frame_status)) return fail(FLACMI_E_INVALID, "null argument");
    if (bytes < 0 || bytes > ctx->frames_bytes || (bytes > 0 && !out))
        return fail(FLACMI_E_INVALID, "the last flacmi_recompress_host call holds %lld bytes", (long long)ctx->frames_bytes);
    memcpy(frame_offsets, ctx->rc_offsets.data(), sizeof(int64_t) * ((size_t)n_blocks + 1));
    if (n_blocks > 0) memcpy(frame_status, ctx->rc_status.data(), sizeof(int32_t) * (size_t)n_blocks);
    if (bytes == 0) return 0;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipMemcpy(out, ctx->h_frames.p, (size_t)bytes, hipMemcpyDeviceToHost));
    return 0;
}

/* ---- pipelined host encode ---------------------------------------------------------
 * Streams: `cs` = the context's stream (compute: analysis, sizes, k_export of the offsets /
 * status into mapped host memory, pack, in order, so the context's shared scratch is never used by two launches
 * at once), `is`
 * (host -> device samples) and `os` (device -> host frame bytes).  Per sub-batch k (slot
 * k % kEncSlots):
 *   front(k): is: H2D rows -> cs: analyze, frame sizes, k_export (offsets/status to host)
 *   back(k):  host waits for those offsets, then cs: pack -> os: frame bytes D2H into out
 * issued as front(0), front(1), back(0), front(2), back(1), ... so the copies of one
 * sub-batch run under the kernels of the others.  The offsets of k are written by a kernel
 * into mapped host memory: as a DMA copy they queued behind the frame bytes of k - 1 and
 * the host waited for that copy before issuing the next H2D (the two copy directions then
 * ran back to back).
 * Streams, events, slot buffers and the pinned offset arrays live in the context and grow
 * as needed (ensure_buf), so streaming many calls pays no setup. */
namespace {
constexpr int kEncSlots = 4; /* with 3 the host waited for the D2H of sub-batch k - 3 before issuing the H2D of k */
struct EncSlot {
    DevBuf samples, meta, params, residual, offsets, status, frames;
    DevBuf subkind;             /* sub_kind of the sub-batch's units (FLACMI_FRAME_FALLBACK) */
    DevBuf wasted;              /* wasted bits of the sub-batch's units (FLACMI_FRAME_WASTED) */
    DevBuf side, choice;        /* side rows and per-frame choice of the sub-batch (FLACMI_STEREO_BEST) */
    int64_t* h_off = nullptr;   /* pinned, mapped: frame offsets of the sub-batch */
    int32_t* h_st = nullptr;    /* pinned, mapped: frame status */
    int64_t* d_off = nullptr;   /* their device-side addresses (k_export writes them) */
    int32_t* d_st = nullptr;
    hipEvent_t e[9] = {};       /* h2d start/end, analyze end, sizes end, pack start/end, d2h start/end, offsets copied */
    flacmi_batch b{};
    int64_t first_unit = 0, nf = 0, total = 0, dstride = 0;
    int rbytes = 4;
};
float ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}
}  // namespace

struct EncState {
    hipStream_t is = nullptr, os = nullptr; /* compute runs on the context's stream */
    EncSlot slot[kEncSlots];
    int64_t cap_nf = 0; /* frames the pinned arrays of each slot hold */
};

static hipStream_t enc_side(flacmi_ctx* ctx) { return ctx->enc ? ctx->enc->is : nullptr; }

static void enc_free(EncState* es) {
    if (!es) return;
    for (hipStream_t st : {es->is, es->os})
        if (st) (void)hipStreamSynchronize(st);
    for (auto& sl : es->slot) {
        for (DevBuf* d : {&sl.samples, &sl.meta, &sl.params, &sl.residual, &sl.offsets, &sl.status, &sl.frames,
                          &sl.subkind, &sl.side, &sl.choice, &sl.wasted})
            if (d->p) (void)hipFree(d->p);
        if (sl.h_off) (void)hipHostFree(sl.h_off);
        if (sl.h_st) (void)hipHostFree(sl.h_st);
        for (auto& e : sl.e)
            if (e) (void)hipEventDestroy(e);
    }
    for (hipStream_t st : {es->is, es->os})
        if (st) (void)hipStreamDestroy(st);
    delete es;
}

/* The pipeline's streams, created on first use and kept for the context's lifetime.  The
 * overlap mode of analyze_device_impl borrows `is` for its k_lpc launches, so no call creates
 * or destroys a stream of its own (a process holds GPU_MAX_HW_QUEUES hardware queues). */
static int enc_streams(flacmi_ctx* ctx) {
    if (!ctx->enc) {
        /* built whole before it is published: a failed create leaves no half state behind */
        EncState* es = new EncState();
        hipError_t e = hipStreamCreateWithFlags(&es->is, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&es->os, hipStreamNonBlocking);
        for (auto& sl : es->slot)
            for (auto& ev : sl.e)
                if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e != hipSuccess) {
            enc_free(es);
            return fail(FLACMI_E_HIP, "encode pipeline state: %s", hipGetErrorString(e));
        }
        ctx->enc = es;
    }
    return 0;
}

static int enc_state(flacmi_ctx* ctx, int64_t per_nf, EncState** out) {
    if (int rc = enc_streams(ctx)) return rc;
    EncState* es = ctx->enc;
    if (es->cap_nf < per_nf) {
        for (auto& sl : es->slot) {
            if (sl.h_off) HIP_TRY(hipHostFree(sl.h_off));
            if (sl.h_st) HIP_TRY(hipHostFree(sl.h_st));
            sl.h_off = nullptr;
            sl.h_st = nullptr;
        }
        es->cap_nf = 0;
        for (auto& sl : es->slot) {
            HIP_TRY(hipHostMalloc((void**)&sl.h_off, sizeof(int64_t) * (per_nf + 1), hipHostMallocMapped | hipHostMallocCoherent));
            HIP_TRY(hipHostMalloc((void**)&sl.h_st, sizeof(int32_t) * per_nf, hipHostMallocMapped | hipHostMallocCoherent));
            HIP_TRY(hipHostGetDevicePointer((void**)&sl.d_off, sl.h_off, 0));
            HIP_TRY(hipHostGetDevicePointer((void**)&sl.d_st, sl.h_st, 0));
        }
        es->cap_nf = per_nf;
    }
    *out = es;
    return 0;
}

static int enc_front(flacmi_ctx* ctx, EncSlot& sl, const flacmi_batch* whole, const flacmi_params* params,
                     const flacmi_frame_params* fp, hipStream_t cs, hipStream_t is) {
    const flacmi_batch& b = sl.b;
    const size_t nu = (size_t)b.n_units;
    /* rows already at the padded device stride go as one linear copy; any other stride (a
       row view of a wider array) is packed to padded device rows by a 2-D copy */
    const int64_t padded = row_pitch(b.block_len, b.sample_bytes);
    const bool linear = whole->unit_stride == padded;
    sl.dstride = padded;
    const int64_t sstride = sl.dstride;
    const int64_t pstride = (1LL << (params->rice_max > 0 ? params->rice_max : 0)) + 1;
    const int64_t rstride = ((b.block_len * sl.rbytes + 15) / 16) * 16 / sl.rbytes;
    const size_t nou = stereo_out_units(fp, nu); /* units of the analysis outputs */
    if (int rc = ensure_buf(sl.samples, stereo_sample_rows(fp, nu) * sstride * b.sample_bytes)) return rc;
    if (int rc = ensure_buf(sl.meta, nou * sizeof(flacmi_unit_meta))) return rc;
    if (int rc = ensure_buf(sl.params, nou * pstride * sizeof(int32_t))) return rc;
    if (int rc = ensure_buf(sl.residual, nou * rstride * sl.rbytes)) return rc;
    if (int rc = ensure_buf(sl.offsets, sizeof(int64_t) * (size_t)(sl.nf + 1))) return rc;
    if (int rc = ensure_buf(sl.status, sizeof(int32_t) * (size_t)sl.nf)) return rc;
    const uint8_t* src = (const uint8_t*)whole->samples + sl.first_unit * whole->unit_stride * b.sample_bytes;
    HIP_TRY(hipEventRecord(sl.e[0], is));
    if (linear)
        HIP_TRY(hipMemcpyAsync(sl.samples.p, src, ((nu - 1) * sstride + b.block_len) * b.sample_bytes,
                               hipMemcpyHostToDevice, is));
    else
        HIP_TRY(hipMemcpy2DAsync(sl.samples.p, sstride * b.sample_bytes, src, whole->unit_stride * b.sample_bytes,
                                 b.block_len * b.sample_bytes, nu, hipMemcpyHostToDevice, is));
    HIP_TRY(hipEventRecord(sl.e[1], is));
    HIP_TRY(hipStreamWaitEvent(cs, sl.e[1], 0));
    flacmi_batch db = b;
    db.samples = sl.samples.p;
    db.unit_stride = sstride;
    /* on the rows this call has just copied (a redo with 8-byte residual rows copies them again) */
    if (int rc = wasted_shift(fp, db, sl.wasted, cs)) return rc;
    flacmi_outputs o{};
    o.meta = (flacmi_unit_meta*)sl.meta.p;
    o.rice_params = (int32_t*)sl.params.p;
    o.params_stride = pstride;
    o.residual = sl.residual.p;
    o.residual_bytes = sl.rbytes;
    o.residual_stride = rstride;
    /* no chunk overlap inside the pipeline: its side stream is this pipeline's H2D stream,
       and the next sub-batch's copy would queue behind this one's k_lpc */
    if (stereo_on(fp)) {
        if (int rc = stereo_analyze(ctx, db, params, o, sl.side, cs, false)) return rc;
    } else {
        if (int rc = validate(&db, params, &o)) return rc;
        if (int rc = analyze_device_impl(ctx, &db, params, &o, cs, false)) return rc;
    }
    HIP_TRY(hipEventRecord(sl.e[2], cs));
    flacmi_frame_params f = *fp;
    f.first_frame = fp->first_frame + sl.first_unit / fp->channels;
    FrameArgs a = frame_args(ctx, &db, &f, o.meta, o.rice_params, pstride, sl.nf);
    if (int rc = stereo_args(fp, db, sl.side, sl.choice, a)) return rc;
    if (int rc = own_sub_kind(fp, sl.subkind, a)) return rc;
    wasted_args(fp, sl.wasted, a);
    if (int rc = frame_sizes_impl(ctx, a, (int64_t*)sl.offsets.p, (int32_t*)sl.status.p, cs)) return rc;
    HIP_TRY(hipEventRecord(sl.e[3], cs));
    HIP_TRY(launch_export((const int64_t*)sl.offsets.p, (const int32_t*)sl.status.p, sl.nf, sl.d_off, sl.d_st, cs));
    HIP_TRY(hipEventRecord(sl.e[8], cs));
    return 0;
}

extern "C" int flacmi_host_register(flacmi_ctx* ctx, void* ptr, size_t bytes) {
    if (!ctx || !ptr || bytes == 0) return fail(FLACMI_E_INVALID, "null context, pointer or empty range");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return 0;
}

extern "C" int flacmi_host_unregister(flacmi_ctx* ctx, void* ptr) {
    if (!ctx || !ptr) return fail(FLACMI_E_INVALID, "null context or pointer");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipHostUnregister(ptr));
    return 0;
}

extern "C" void* flacmi_host_alloc(flacmi_ctx* ctx, size_t bytes) {
    if (!ctx || bytes == 0) {
        fail(FLACMI_E_INVALID, "null context or empty range");
        return nullptr;
    }
    if (set_device(ctx)) return nullptr;
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        fail(FLACMI_E_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

extern "C" int flacmi_host_free(flacmi_ctx* ctx, void* ptr) {
    if (!ptr) return 0;
    if (ctx)
        if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipHostFree(ptr));
    return 0;
}

extern "C" int flacmi_encode_pipeline(flacmi_ctx* ctx, const flacmi_batch* batch, const flacmi_params* params,
                                      const flacmi_frame_params* fp, int64_t units_per_batch, uint8_t* out,
                                      int64_t out_capacity, int64_t* frame_offsets, int32_t* frame_status,
                                      flacmi_encode_timing* timing) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    int64_t nf = 0;
    if (int rc = validate_frames(batch, fp, &nf)) return rc;
    if (!params || !frame_offsets || !frame_status || (!out && out_capacity > 0))
        return fail(FLACMI_E_INVALID, "null argument");
    flacmi_params sized;
    if (int rc = size_choice_params(params, fp, &sized)) return rc;
    params = &sized;
    const int C = fp->channels;
    if (units_per_batch < C || units_per_batch % C) return fail(FLACMI_E_INVALID, "units_per_batch must be a positive multiple of channels");
    if (batch->unit_stride < batch->block_len) return fail(FLACMI_E_INVALID, "unit_stride < block_len");
    flacmi_encode_timing t{};
    const auto w0 = std::chrono::steady_clock::now();
    frame_offsets[0] = 0;
    if (nf == 0) {
        if (timing) *timing = t;
        return 0;
    }
    if (int rc = set_device(ctx)) return rc;
    units_per_batch = std::min(units_per_batch, ((batch->n_units + C - 1) / C) * C);
    EncState* es = nullptr;
    if (int rc = enc_state(ctx, units_per_batch / C, &es)) return rc;
    /* the caller's rows and output, page-locked in place for the call */
    const auto r0 = std::chrono::steady_clock::now();
    const size_t in_bytes = (size_t)((batch->n_units - 1) * batch->unit_stride + batch->block_len) * batch->sample_bytes;
    /* a buffer already page-locked (flacmi_host_register, flacmi_host_alloc) is used as it is */
    auto locked = [](const void* q) {
        hipPointerAttribute_t at{};
        const bool y = hipPointerGetAttributes(&at, q) == hipSuccess && at.type == hipMemoryTypeHost;
        (void)hipGetLastError();
        return y;
    };
    const bool reg_in = !locked(batch->samples) &&
                        hipHostRegister(const_cast<void*>(batch->samples), in_bytes, hipHostRegisterDefault) == hipSuccess;
    const bool reg_out = out_capacity > 0 && !locked(out) &&
                         hipHostRegister(out, (size_t)out_capacity, hipHostRegisterDefault) == hipSuccess;
    (void)hipGetLastError();
    t.register_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r0).count();
    /* three streams in all (with the null stream four: GPU_MAX_HW_QUEUES' default).  With a
     * fifth the runtime maps two streams onto one hardware queue, and the copies of the two
     * directions then wait for each other in submission order (measured: H2D of sub-batch
     * k + 2 started only when the D2H of k had finished). */
    hipStream_t cs = ctx->stream, is = es->is, os = es->os;
    EncSlot* slot = es->slot;
    int rc = 0;
    {
        const int64_t nsub = (batch->n_units + units_per_batch - 1) / units_per_batch;
        auto setup = [&](int64_t k) {
            EncSlot& sl = slot[k % kEncSlots];
            sl.first_unit = k * units_per_batch;
            const int64_t nu = std::min(units_per_batch, batch->n_units - sl.first_unit);
            sl.b = *batch;
            sl.b.n_units = nu;
            sl.b.n_tail_units = (sl.first_unit + nu == batch->n_units) ? batch->n_tail_units : 0;
            sl.nf = nu / C;
            sl.rbytes = 4;
        };
        int64_t written = 0; /* frame bytes of the sub-batches already placed */
        auto back = [&](int64_t k) -> int {
            EncSlot& sl = slot[k % kEncSlots];
            HIP_TRY(hipEventSynchronize(sl.e[8])); /* the offsets / status of sub-batch k */
            bool wide = false;
            for (int64_t f = 0; f < sl.nf && sl.rbytes == 4; ++f)
                if ((sl.h_st[f] & 0xffff) == FLACMI_STATUS_RESIDUAL_WIDE) wide = true;
            if (wide) { /* a chosen residual needs 64 bits: redo this sub-batch with 8-byte rows */
                sl.rbytes = 8;
                if (int r = enc_front(ctx, sl, batch, params, fp, cs, is)) return r;
                HIP_TRY(hipEventSynchronize(sl.e[8]));
            }
            sl.total = sl.h_off[sl.nf];
            const int64_t f0 = sl.first_unit / C;
            for (int64_t f = 0; f < sl.nf; ++f) {
                frame_offsets[f0 + f + 1] = written + sl.h_off[f + 1];
                frame_status[f0 + f] = sl.h_st[f];
            }
            if (written + sl.total > out_capacity)
                return fail(FLACMI_E_NOMEM, "frames need %lld bytes, out holds %lld", (long long)(written + sl.total),
                            (long long)out_capacity);
            if (int r = ensure_buf(sl.frames, (size_t)sl.total + 16)) return r;
            const int64_t pstride = (1LL << (params->rice_max > 0 ? params->rice_max : 0)) + 1;
            const int64_t rstride = ((sl.b.block_len * sl.rbytes + 15) / 16) * 16 / sl.rbytes;
            flacmi_batch db = sl.b;
            db.samples = sl.samples.p;
            db.unit_stride = sl.dstride;
            flacmi_frame_params f = *fp;
            f.first_frame = fp->first_frame + f0;
            FrameArgs a = frame_args(ctx, &db, &f, (const flacmi_unit_meta*)sl.meta.p, (const int32_t*)sl.params.p,
                                     pstride, sl.nf);
            if (int r = stereo_args(fp, db, sl.side, sl.choice, a)) return r; /* what enc_front's kernels wrote */
            if (int r = own_sub_kind(fp, sl.subkind, a)) return r; /* the array enc_front's k_sub_kinds wrote */
            wasted_args(fp, sl.wasted, a); /* and the one its k_wasted_rows wrote */
            a.residual = sl.residual.p;
            a.residual_bytes = sl.rbytes;
            a.residual_stride = rstride;
            a.offsets = (int64_t*)sl.offsets.p;
            a.status = (int32_t*)sl.status.p;
            a.out = (uint8_t*)sl.frames.p;
            a.capacity = sl.total;
            if (int r = pack_lists(ctx, a)) return r;
            HIP_TRY(hipEventRecord(sl.e[4], cs));
            HIP_TRY(launch_pack(a, cs));
            HIP_TRY(hipEventRecord(sl.e[5], cs));
            HIP_TRY(hipStreamWaitEvent(os, sl.e[5], 0));
            HIP_TRY(hipEventRecord(sl.e[6], os));
            if (sl.total > 0)
                HIP_TRY(hipMemcpyAsync(out + written, sl.frames.p, (size_t)sl.total, hipMemcpyDeviceToHost, os));
            HIP_TRY(hipEventRecord(sl.e[7], os));
            written += sl.total;
            t.bytes_out += sl.total;
            return 0;
        };
        /* diagnostic (FLACMI_ENC_TRACE): per-sub-batch timeline in ms from the call's start */
        hipEvent_t tb = nullptr;
        static const bool trace = std::getenv("FLACMI_ENC_TRACE") != nullptr; /* read once */
        if (trace && hipEventCreate(&tb) == hipSuccess) (void)hipEventRecord(tb, is);
        auto account = [&](int64_t k) {
            EncSlot& sl = slot[k % kEncSlots];
            (void)hipEventSynchronize(sl.e[7]);
            if (tb)
                std::fprintf(stderr, "enc %lld: h2d %.2f-%.2f an-end %.2f sz-end %.2f off %.2f pack %.2f-%.2f d2h %.2f-%.2f\n",
                             (long long)k, ev_ms(tb, sl.e[0]), ev_ms(tb, sl.e[1]), ev_ms(tb, sl.e[2]), ev_ms(tb, sl.e[3]),
                             ev_ms(tb, sl.e[8]), ev_ms(tb, sl.e[4]), ev_ms(tb, sl.e[5]), ev_ms(tb, sl.e[6]), ev_ms(tb, sl.e[7]));
            t.h2d_ms += ev_ms(sl.e[0], sl.e[1]);
            t.analyze_ms += ev_ms(sl.e[1], sl.e[2]);
            t.sizes_ms += ev_ms(sl.e[2], sl.e[3]);
            t.pack_ms += ev_ms(sl.e[4], sl.e[5]);
            t.d2h_ms += ev_ms(sl.e[6], sl.e[7]);
            t.bytes_in += (int64_t)sl.b.n_units * sl.b.block_len * sl.b.sample_bytes;
        };
        for (int64_t k = 0; k < nsub; ++k) {
            if (k >= kEncSlots) account(k - kEncSlots); /* the slot is free once those frames are copied */
            setup(k);
            if ((rc = enc_front(ctx, slot[k % kEncSlots], batch, params, fp, cs, is))) break;
            if (k >= 1 && (rc = back(k - 1))) break;
        }
        if (!rc && (rc = back(nsub - 1)) == 0)
            for (int64_t k = (nsub >= kEncSlots ? nsub - kEncSlots : 0); k < nsub; ++k) account(k);
        t.sub_batches = nsub;
        if (tb) (void)hipEventDestroy(tb);
    }
    /* nothing may still read the caller's rows or write its buffer once this returns */
    for (hipStream_t st : {cs, is, os}) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess && !rc) rc = fail(FLACMI_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    }
    {
        const auto u0 = std::chrono::steady_clock::now();
        if (reg_in) (void)hipHostUnregister(const_cast<void*>(batch->samples));
        if (reg_out) (void)hipHostUnregister(out);
        t.register_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
    }
    t.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    if (timing) *timing = t;
    return rc;
}

int flacmi_encode_fetch(flacmi_ctx* ctx, uint8_t* out, int64_t bytes) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (bytes < 0 || bytes > ctx->frames_bytes) return fail(FLACMI_E_INVALID, "at most %lld bytes are held",
                                                            (long long)ctx->frames_bytes);
    if (bytes == 0) return 0;
    if (!out) return fail(FLACMI_E_INVALID, "null output");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipMemcpy(out, ctx->h_frames.p, (size_t)bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

extern "C" {

int flacmi_stream_stats(flacmi_ctx* ctx, const flacmi_unit_meta* d_meta, int64_t n_units, int32_t block_len,
                        int32_t tail_len, int64_t n_tail_units, int64_t* d_stats, void* stream) {
    if (!ctx || !d_stats) return fail(FLACMI_E_INVALID, "null argument");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * FLACMI_STATS_WORDS, (hipStream_t)stream));
    HIP_TRY(launch_stats(d_meta, n_units, block_len, tail_len, n_tail_units, d_stats, (hipStream_t)stream));
    return 0;
}

/* ---- RCCL stats reduce: librccl.so.1 is opened on first use (no link-time dependency, so
 * the product library loads where RCCL is absent; a process that already loaded RCCL, e.g.
 * through torch, gets the same library back from dlopen) ---- */
namespace {
struct Rccl {
    void* h = nullptr;
    int (*get_id)(void* id) = nullptr;
    int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*destroy)(void*) = nullptr;
    const char* (*err)(int) = nullptr;
};
struct RcclId {
    char b[FLACMI_COMM_ID_BYTES];
};
/* ncclCommInitRank takes the 128-byte ncclUniqueId by value */
typedef int (*rccl_init_rank_t)(void** comm, int nranks, RcclId id, int rank);
Rccl g_rccl;
rccl_init_rank_t g_rccl_init = nullptr;
std::mutex g_rccl_mu;
constexpr int kNcclInt64 = 4, kNcclSum = 0; /* ncclDataType_t ncclInt64, ncclRedOp_t ncclSum */

int rccl_load() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.h) return 0;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(FLACMI_E_UNSUPPORTED, "librccl.so.1 not found: %s", dlerror());
    Rccl r;
    r.h = h;
    r.get_id = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
    g_rccl_init = (rccl_init_rank_t)dlsym(h, "ncclCommInitRank");
    r.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
    r.destroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    r.err = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!r.get_id || !g_rccl_init || !r.all_reduce || !r.destroy || !r.err)
        return fail(FLACMI_E_UNSUPPORTED, "librccl.so.1 lacks an entry point");
    g_rccl = r;
    return 0;
}
int rccl_fail(const char* what, int rc) {
    return fail(FLACMI_E_HIP, "%s: RCCL error %d (%s)", what, rc, g_rccl.err ? g_rccl.err(rc) : "?");
}
}  // namespace

struct flacmi_comm {
    flacmi_ctx* ctx;
    void* comm; /* ncclComm_t */
    int nranks, rank;
};

int flacmi_comm_available(void) { return rccl_load(); }

int64_t flacmi_unit_stride(int32_t block_len, int32_t sample_bytes) {
    if (block_len < 1 || (sample_bytes != 2 && sample_bytes != 4)) return fail(FLACMI_E_INVALID, "block_len < 1 or sample_bytes not 2/4");
    return row_pitch(block_len, sample_bytes);
}

int flacmi_comm_id(void* id_out) {
    if (!id_out) return fail(FLACMI_E_INVALID, "null argument");
    if (int rc = rccl_load()) return rc;
    if (int rc = g_rccl.get_id(id_out)) return rccl_fail("ncclGetUniqueId", rc);
    return 0;
}

int flacmi_comm_init(flacmi_ctx* ctx, int nranks, int rank, const void* id, flacmi_comm** out) {
    if (!ctx || !id || !out) return fail(FLACMI_E_INVALID, "null argument");
    *out = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(FLACMI_E_INVALID, "rank %d of %d", rank, nranks);
    if (int rc = rccl_load()) return rc;
    if (int rc = set_device(ctx)) return rc;
    RcclId cid;
    memcpy(cid.b, id, FLACMI_COMM_ID_BYTES);
    void* c = nullptr;
    if (int rc = g_rccl_init(&c, nranks, cid, rank)) return rccl_fail("ncclCommInitRank", rc);
    *out = new flacmi_comm{ctx, c, nranks, rank};
    return 0;
}

int flacmi_allreduce_stats(flacmi_comm* comm, int64_t* d_stats, void* stream) {
    if (!comm || !d_stats) return fail(FLACMI_E_INVALID, "null argument");
    if (int rc = set_device(comm->ctx)) return rc;
    if (int rc = g_rccl.all_reduce(d_stats, d_stats, FLACMI_STATS_WORDS, kNcclInt64, kNcclSum, comm->comm,
                                   (hipStream_t)stream))
        return rccl_fail("ncclAllReduce", rc);
    return 0;
}

int flacmi_comm_destroy(flacmi_comm* comm) {
    if (!comm) return 0;
    int rc = 0;
    if (comm->comm && g_rccl.destroy) {
        if (int e = set_device(comm->ctx)) rc = e;
        if (int e = g_rccl.destroy(comm->comm)) rc = rccl_fail("ncclCommDestroy", e);
    }
    delete comm;
    return rc;
}

int flacmi_synth_mix_device(flacmi_ctx* ctx, void* dst, int32_t sample_bytes, int32_t sample_bits,
                            int64_t unit_stride, int64_t first_unit, int64_t n_units, int32_t len, uint64_t seed,
                            int32_t open_eighths, void* stream) {
    if (!ctx || !dst) return fail(FLACMI_E_INVALID, "null argument");
    if (sample_bytes != 2 && sample_bytes != 4) return fail(FLACMI_E_INVALID, "sample_bytes must be 2 or 4");
    if (sample_bits < 8 || sample_bits > 8 * sample_bytes || (sample_bits > 16 && sample_bits - 16 > 15))
        return fail(FLACMI_E_INVALID, "sample_bits out of range");
    if (len < 1 || unit_stride < len) return fail(FLACMI_E_INVALID, "bad length/stride");
    if (n_units > 0x7fffffff) return fail(FLACMI_E_INVALID, "at most 2^31-1 units per synth call");
    if (open_eighths < 0 || open_eighths > 8) return fail(FLACMI_E_INVALID, "open_eighths must be 0..8");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(launch_synth(dst, sample_bytes, sample_bits, unit_stride, first_unit, n_units, len, seed, ctx->d_sintab,
                         open_eighths, (hipStream_t)stream));
    return 0;
}

int flacmi_synth_device(flacmi_ctx* ctx, void* dst, int32_t sample_bytes, int32_t sample_bits, int64_t unit_stride,
                        int64_t first_unit, int64_t n_units, int32_t len, uint64_t seed, void* stream) {
    return flacmi_synth_mix_device(ctx, dst, sample_bytes, sample_bits, unit_stride, first_unit, n_units, len, seed, 0,
                                   stream);
}

void* flacmi_device_alloc(flacmi_ctx* ctx, size_t bytes) {
    if (!ctx) return nullptr;
    if (set_device(ctx)) return nullptr;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        fail(FLACMI_E_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

int flacmi_device_free(flacmi_ctx* ctx, void* ptr) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipFree(ptr));
    return 0;
}

int flacmi_memcpy_h2d(flacmi_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

int flacmi_memcpy_d2h(flacmi_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int flacmi_synchronize(flacmi_ctx* ctx) {
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

int flacmi_last_timing(flacmi_ctx* ctx, float* ms, int n) {
    if (!ctx || ctx->ncalls == 0) return fail(FLACMI_E_INVALID, "no timed call");
    if (int rc = set_device(ctx)) return rc;
    const int k = ctx->ncalls < flacmi_ctx::kRing ? ctx->ncalls : flacmi_ctx::kRing;
    double acc[3] = {0, 0, 0};
    for (int c = ctx->ncalls - k; c < ctx->ncalls; ++c) {
        hipEvent_t* ev = ctx->ev[c % flacmi_ctx::kRing];
        HIP_TRY(hipEventSynchronize(ev[2]));
        float t;
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        acc[0] += t;
        const int nk = ctx->nchunks[c % flacmi_ctx::kRing];
        if (nk == 0) {
            HIP_TRY(hipEventElapsedTime(&t, ev[1], ev[2]));
            acc[1] += t;
        } else { /* overlap: the k_resid launches' own spans */
            for (int i = 0; i < nk; ++i) {
                HIP_TRY(hipEventElapsedTime(&t, ev[3 + 2 * i], ev[4 + 2 * i]));
                acc[1] += t;
            }
        }
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[2]));
        acc[2] += t;
    }
    const float vals[4] = {(float)(acc[0] / k), (float)(acc[1] / k), (float)(acc[2] / k), (float)k};
    const int m = n < 4 ? n : 4;
    for (int i = 0; i < m; ++i) ms[i] = vals[i];
    return m;
}

int flacmi_timing_reset(flacmi_ctx* ctx) {
    if (!ctx) return fail(FLACMI_E_INVALID, "null context");
    ctx->ncalls = 0;
    return 0;
}

double flacmi_host_pypow2(double x, int32_t* status) {
    static const uint64_t lh[] = GLIBC_POW_LOG_HDR, lt[] = GLIBC_POW_LOG_TAB, eh[] = GLIBC_EXP_HDR,
                          et[] = GLIBC_EXP_TAB;
    const pym::PowTables T{lh, lt, eh, et};
    int st = 0;
    const double r = pym::py_pow2(x, T, &st);
    if (status) *status = st;
    return r;
}

int32_t flacmi_host_floor_log2(double x) {
    ensure_tables();
    if (!(x > 0.0) || std::isinf(x)) return INT32_MIN; /* outside the domain (the table covers finite x > 0) */
    return pym::py_floor_log2(x, g_log2thr.data());
}

int flacmi_device_selftest(flacmi_ctx* ctx, int32_t which, const double* x, double* out, int32_t* status,
                           int64_t n) {
    if (!ctx || !x || !out || !status) return fail(FLACMI_E_INVALID, "null argument");
    if (which != 0 && which != 1) return fail(FLACMI_E_INVALID, "which must be 0 or 1");
    if (n <= 0) return 0;
    if (int rc = set_device(ctx)) return rc;
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)n * (8 + 8 + 4)));
    double* dx = (double*)d;
    double* dout = dx + n;
    int32_t* dst = (int32_t*)(dout + n);
    int rc = 0;
    hipError_t e = hipMemcpyAsync(dx, x, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_selftest(which, dx, dout, dst, n, ctx->d_log2thr, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(status, dst, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = fail(FLACMI_E_HIP, "selftest: %s", hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
}

int flacmi_device_lpc_from_acf(flacmi_ctx* ctx, const double* acf, int64_t n, int32_t L, int32_t q, int32_t* rec) {
    if (!ctx || !acf || !rec) return fail(FLACMI_E_INVALID, "null argument");
    if (L < 1 || L > FLACMI_MAX_LPC_ORDER) return fail(FLACMI_E_INVALID, "L must be in 1..%d", FLACMI_MAX_LPC_ORDER);
    if (q < 5 || q > 15) return fail(FLACMI_E_INVALID, "q must be in 5..15");
    if (n <= 0) return 0;
    if (int rc = set_device(ctx)) return rc;
    const int rw = FLACMI_LPC_REC_WORDS(L);
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)n * (33 * 8 + (size_t)rw * 4)));
    LpcArgs a{};
    a.acf = (double*)d;
    a.rec = (int32_t*)(a.acf + n * 33);
    a.count = n;
    a.n = 1 << 12;
    a.L = L;
    a.q = q;
    a.rec_words = rw;
    a.log2thr = ctx->d_log2thr;
    int rc = 0;
    hipError_t e = hipMemcpyAsync(a.acf, acf, (size_t)n * 33 * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_lpc_from_acf(a, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(rec, a.rec, (size_t)n * rw * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = fail(FLACMI_E_HIP, "lpc_from_acf: %s", hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
