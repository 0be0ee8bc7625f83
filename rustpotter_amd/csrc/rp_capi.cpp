// rp_capi.cpp -- extern "C" surface declared in include/rustpotter_hip.h.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <system_error>
#include <chrono>
#include <thread>

#include "rp_capi.h"

namespace rp { const std::string &last_error(); }

using namespace rp;

struct rp_detector {
    std::unique_ptr<Rustpotter> impl;
    // storage backing the last rp_detection handed out
    Detection last;
    std::vector<const char *> name_ptrs;
};

static void fill_detection(rp_detector *d, const Detection &src, rp_detection *out) {
    d->last = src;
    d->name_ptrs.clear();
    for (auto &s : d->last.score_names) d->name_ptrs.push_back(s.c_str());
    out->name = d->last.name.c_str();
    out->avg_score = d->last.avg_score;
    out->score = d->last.score;
    out->n_scores = d->last.scores.size();
    out->score_names = d->name_ptrs.data();
    out->scores = d->last.scores.data();
    out->counter = d->last.counter;
    out->gain = d->last.gain;
}

namespace rp {

int frontend_batch(Ctx *c, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride, const rp_filters_config *filters,
                   float rms_level_ref, size_t window_size, const Bank *bank, const int32_t *stream_wakeword, float *pcm_out, size_t out_stride,
                   float *rms, float *gains, const TargetSide *sides) {
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
    if (pcm_stride < n_samples || out_stride < n_samples) { set_last_error("stride smaller than n_samples"); return -1; }
    if (!sample_format_ok(fmt)) return -1;
    if (!filters) { set_last_error("null argument"); return -1; }
    const rp_gain_normalization_config &g = filters->gain_normalizer;
    const rp_band_pass_config &b = filters->band_pass;
    if (bank) window_size = (size_t)std::max(bank->dev.max_len / 3, 1);   // the ring's capacity: the bank's largest window (src/detector.rs:337)
    else if (!sides && g.enabled && g.has_gain_ref) rms_level_ref = g.gain_ref;   // fixed_rms_level, gain_normalizer_filter.rs:56-66
    // (sides: window_size is the caller's, the largest window of the banks the rows index)
    if (window_size == 0) window_size = 1;                                // set_rms_level_ref :47
    if (window_size > 1u << 20) { set_last_error("window_size too large"); return -1; }
    float q[5];
    band_pass_coefficients(b, q);
    const float a0 = q[0], a1 = q[1], a2 = q[2], b1 = q[3], b2 = q[4];
    const size_t n_chunks = n_samples / 480;
    Staged sg(c);
    PerStreamGain per;
    if (bank) {  // a refused index: before anything is launched or written
        BankIndices bi;
        if (!stage_bank_indices(c, sg, *bank, stream_wakeword, S, 0, 0, &bi)) return -1;
        per.stream_wakeword = bi.dev;
        per.ww = bank->dev.ww; per.rms_level = bank->rms_level; per.W = bank->dev.W;
        per.has_fixed_ref = g.has_gain_ref ? 1 : 0; per.fixed_ref = g.gain_ref;
    }
    if (sides) {  // the staged DEVICE rows of one bank, or of references and of models: every stream's level and window, prepared in front of the gain kernel
        if (!c->ws_gain_tab.reserve(gain_targets_bytes(S))) return -1;
        if (!hip_ok(launch_stream_targets(c->stream, sides[0], sides[1], S, c->ws_gain_tab.p, &per), "stream_targets_kernel")) return -1;
        per.has_fixed_ref = g.has_gain_ref ? 1 : 0; per.fixed_ref = g.gain_ref;
    }
    const void *dp = sg.in(pcm, S * pcm_stride * sample_bytes(fmt), c->stage_in);
    float *dout = static_cast<float *>(sg.out(pcm_out, S * out_stride * sizeof(float), c->stage_out));
    if (S && (!dp || !dout)) { if (!pcm || !pcm_out) set_last_error("null argument"); return -1; }
    if (!c->ws_rms.reserve(S * n_chunks * 4 + 16) || !c->ws_gain.reserve(S * n_chunks * 4 + 16) ||
        !c->ws_ring.reserve(S * window_size * 4 + 16)) return -1;
    const hipError_t e = bank || sides ? launch_frontend_per_stream(c->stream, dp, (int)fmt, S, n_samples, pcm_stride, g.enabled ? 1 : 0, per, (int)window_size,
                                                           g.min_gain, g.max_gain, b.enabled ? 1 : 0, a0, a1, a2, b1, b2, c->ws_ring.as<float>(),
                                                           c->ws_rms.as<float>(), c->ws_gain.as<float>(), dout, out_stride)
                              : launch_frontend(c->stream, dp, (int)fmt, S, n_samples, pcm_stride, g.enabled ? 1 : 0, rms_level_ref, g.min_gain,
                                                g.max_gain, (int)window_size, b.enabled ? 1 : 0, a0, a1, a2, b1, b2, c->ws_ring.as<float>(),
                                                c->ws_rms.as<float>(), c->ws_gain.as<float>(), dout, out_stride);
    if (!hip_ok(e, "front-end kernels")) return -1;
    auto copy_out = [&](float *dst, const float *src_dev, bool valid) {
        if (!dst) return true;
        if (!valid) {  // gain filter off: every chunk has gain 1
            std::vector<float> ones(S * n_chunks, 1.f);
            return hip_ok(hipMemcpyAsync(dst, ones.data(), ones.size() * 4, sg.host ? hipMemcpyHostToHost : hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync") &&
                   hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        }
        return hip_ok(hipMemcpyAsync(dst, src_dev, S * n_chunks * 4, sg.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync");
    };
    if (!copy_out(rms, c->ws_rms.as<float>(), true) || !copy_out(gains, c->ws_gain.as<float>(), g.enabled)) return -1;
    if (!sg.back(pcm_out, dout, S * out_stride * sizeof(float))) return -1;
    return hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize") ? 0 : -1;
}

}  // namespace rp

extern "C" {

const char *rp_last_error(void) { return last_error().c_str(); }
const char *rp_version(void) { return "rustpotter_hip 0.1.0 (gfx950; mirrors rustpotter 3.0.2)"; }

void rp_config_default(rp_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->fmt.sample_rate = 16000;  // DETECTOR_INTERNAL_SAMPLE_RATE
    c->fmt.sample_format = RP_SAMPLE_F32;
    c->fmt.channels = 1;
    c->fmt.endianness = RP_ENDIAN_LITTLE;
    c->detector.avg_threshold = 0.2f;  // src/constants.rs:4
    c->detector.threshold = 0.5f;      // :5
    c->detector.min_scores = 5;        // :6
    c->detector.eager = false;
    c->detector.score_ref = 0.22f;     // :7
    c->detector.band_size = 5;         // :3
    c->detector.score_mode = RP_SCORE_MAX;
    c->detector.vad_mode = RP_VAD_NONE;
    c->filters.gain_normalizer.enabled = false;
    c->filters.gain_normalizer.has_gain_ref = false;
    c->filters.gain_normalizer.min_gain = 0.1f;
    c->filters.gain_normalizer.max_gain = 1.0f;
    c->filters.band_pass.enabled = false;
    c->filters.band_pass.low_cutoff = 80.f;
    c->filters.band_pass.high_cutoff = 400.f;
}

int rp_new(const rp_config *config, rp_detector **out) {
    return guarded([&]() -> int {
        if (!config || !out) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        std::unique_ptr<Rustpotter> r(Rustpotter::create(*config));
        if (!r) return -1;
        rp_detector *d = new rp_detector();
        d->impl = std::move(r);
        *out = d;
        return 0;
    });
}
void rp_free(rp_detector *d) { delete d; }

int rp_add_wakeword_from_buffer(rp_detector *d, const char *key, const uint8_t *buffer, size_t len) {
    if (!d || !key || (!buffer && len)) { set_last_error("null argument"); return -1; }
    return guarded([&]() -> int { return d->impl->add_wakeword_from_buffer(key, buffer, len) ? 0 : -1; });
}
int rp_add_wakeword_from_file(rp_detector *d, const char *key, const char *path) {
    if (!d || !key || !path) { set_last_error("null argument"); return -1; }
    return guarded([&]() -> int { return d->impl->add_wakeword_from_file(key, path) ? 0 : -1; });
}
bool rp_remove_wakeword(rp_detector *d, const char *key) { return d && key && d->impl->remove_wakeword(key); }
bool rp_remove_wakewords(rp_detector *d) { return d && d->impl->remove_wakewords(); }
size_t rp_get_samples_per_frame(const rp_detector *d) { return d ? d->impl->get_samples_per_frame() : 0; }
size_t rp_get_bytes_per_frame(const rp_detector *d) { return d ? d->impl->get_bytes_per_frame() : 0; }
int rp_get_partial_detection(const rp_detector *d, rp_detection *out) {
    if (!d || !out) { set_last_error("null argument"); return -1; }
    const Detection *p = d->impl->get_partial_detection();
    if (!p) return 0;
    fill_detection(const_cast<rp_detector *>(d), *p, out);
    return 1;
}
float rp_get_rms_level(const rp_detector *d) { return d ? d->impl->get_rms_level() : 0.f; }
float rp_get_gain(const rp_detector *d) { return d ? d->impl->get_gain() : 0.f; }
float rp_get_rms_level_ref(const rp_detector *d) { return d ? d->impl->get_rms_level_ref() : 0.f; }

#define RP_PROCESS(call)                                              \
    if (!d) { set_last_error("null handle"); return -1; }             \
    return guarded([&]() -> int {                                     \
        Detection det;                                                \
        int r = (call);                                               \
        if (r == 1 && out) fill_detection(d, det, out);               \
        return r;                                                     \
    })

int rp_process_bytes(rp_detector *d, const uint8_t *b, size_t len, rp_detection *out) { RP_PROCESS(d->impl->process_bytes(b, len, &det)); }
int rp_process_samples_i8(rp_detector *d, const int8_t *s, size_t n, rp_detection *out) { RP_PROCESS(d->impl->process_samples<int8_t>(s, n, &det)); }
int rp_process_samples_i16(rp_detector *d, const int16_t *s, size_t n, rp_detection *out) { RP_PROCESS(d->impl->process_samples<int16_t>(s, n, &det)); }
int rp_process_samples_i32(rp_detector *d, const int32_t *s, size_t n, rp_detection *out) { RP_PROCESS(d->impl->process_samples<int32_t>(s, n, &det)); }
int rp_process_samples_f32(rp_detector *d, const float *s, size_t n, rp_detection *out) { RP_PROCESS(d->impl->process_samples<float>(s, n, &det)); }

int rp_update_config(rp_detector *d, const rp_config *c) {
    if (!d || !c) { set_last_error("null argument"); return -1; }
    d->impl->update_detector_config(c->detector);
    d->impl->update_filters_config(c->filters);
    return 0;
}
int rp_update_detector_config(rp_detector *d, const rp_detector_config *c) {
    if (!d || !c) { set_last_error("null argument"); return -1; }
    d->impl->update_detector_config(*c);
    return 0;
}
int rp_update_filters_config(rp_detector *d, const rp_filters_config *c) {
    if (!d || !c) { set_last_error("null argument"); return -1; }
    d->impl->update_filters_config(*c);
    return 0;
}
void rp_reset(rp_detector *d) { if (d) d->impl->reset(); }

// ------------------------------------------------------------------- batched level
int rp_ctx_new(int device, int flags, rp_ctx **out) {
    return guarded([&]() -> int {
        if (!out) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if ((flags & RP_CTX_ARITH_STRICT_F32) && (flags & RP_CTX_ARITH_FAST_SPLIT)) { set_last_error("RP_CTX_ARITH_STRICT_F32 and RP_CTX_ARITH_FAST_SPLIT exclude each other"); return -1; }
        std::unique_ptr<Ctx> c(Ctx::create(device, flags));
        if (!c) return -1;
        c->arith.mode = (flags & RP_CTX_ARITH_STRICT_F32) ? kArithStrictF32 : (flags & RP_CTX_ARITH_FAST_SPLIT) ? kArithFastSplit : kArithF32Matrix;
        c->arith.ragged = (flags & RP_CTX_RAGGED_MATRIX) ? 1 : 0;
        rp_ctx *h = new rp_ctx();
        h->impl = std::move(c);
        *out = h;
        return 0;
    });
}
void rp_ctx_free(rp_ctx *ctx) { delete ctx; }
int rp_ctx_set_stream(rp_ctx *ctx, void *s) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    ctx->impl->stream = s ? static_cast<hipStream_t>(s) : ctx->impl->own_stream;
    return 0;
}
int rp_ctx_synchronize(rp_ctx *ctx) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    if (!hip_ok(hipSetDevice(ctx->impl->device), "hipSetDevice")) return -1;
    return hip_ok(hipStreamSynchronize(ctx->impl->stream), "hipStreamSynchronize") ? 0 : -1;
}

static_assert(RP_ARITH_F32_MATRIX == kArithF32Matrix && RP_ARITH_STRICT_F32 == kArithStrictF32 && RP_ARITH_FAST_SPLIT == kArithFastSplit, "RP_ARITH_* mirror rp_kernels.h");
int rp_ctx_set_arithmetic(rp_ctx *ctx, int arith, int ragged_matrix) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    if (arith != RP_ARITH_F32_MATRIX && arith != RP_ARITH_STRICT_F32 && arith != RP_ARITH_FAST_SPLIT) { set_last_error("unknown RP_ARITH_* value"); return -1; }
    ctx->impl->arith.mode = arith;
    ctx->impl->arith.ragged = ragged_matrix ? 1 : 0;
    return 0;
}
int rp_ctx_arithmetic(rp_ctx *ctx, int *ragged_matrix) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    if (ragged_matrix) *ragged_matrix = ctx->impl->arith.ragged;
    return ctx->impl->arith.mode;
}

int rp_ctx_dtw_ref_pairs(rp_ctx *ctx, uint64_t *pairs) {
    if (!ctx || !pairs) { set_last_error("null argument"); return -1; }
    Ctx *c = ctx->impl.get();
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice") || !hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return -1;
    unsigned long long v = 0;
    if (!hip_ok(hipMemcpy(&v, dtw_fix_stats(c->dtw_work().fix), sizeof(v), hipMemcpyDeviceToHost), "hipMemcpy(dtw stats)")) return -1;
    *pairs = (uint64_t)v;
    return 0;
}

int rp_ctx_last_window_scores(rp_ctx *ctx, float *out, size_t n) {
    if (!ctx || (n && !out)) { set_last_error("null argument"); return -1; }
    Ctx *c = ctx->impl.get();
    if (c->last_window_scores == 0) { set_last_error("rp_ctx_last_window_scores: this context has made no rp_batch_detect call that left its scores in the workspace"); return -1; }
    if (n > c->last_window_scores) { set_last_error("rp_ctx_last_window_scores: n exceeds what the last call wrote"); return -1; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice") || !hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return -1;
    if (n && !hip_ok(hipMemcpy(out, c->ws_scores.as<float>(), n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(window scores)")) return -1;
    return 0;
}

#ifndef RP_BUILD_ARCH
#define RP_BUILD_ARCH "gfx950"
#endif
#ifndef RP_BUILD_FLAGS_EXTRA
#define RP_BUILD_FLAGS_EXTRA ""
#endif
const char *rp_build_info(void) { return sizeof(RP_BUILD_FLAGS_EXTRA) > 1 ? RP_BUILD_ARCH " +" RP_BUILD_FLAGS_EXTRA : RP_BUILD_ARCH; }

#ifdef RP_MFMA_TRACE   // variant builds only: read the DTW counter block back (tools/r4_mfma_timeline.py)
extern "C" int rp_debug_read_dtw_work(rp_ctx *ctx, uint32_t *dst, size_t words) {
    Ctx *c = ctx->impl.get();
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice") || !hip_ok(hipStreamSynchronize(c->stream), "sync")) return -1;
    return hip_ok(hipMemcpy(dst, c->dtw_work().sched, words * 4, hipMemcpyDeviceToHost), "hipMemcpy") ? 0 : -1;
}
#endif

int rp_ctx_dtw_kernels(rp_ctx *ctx) {
    if (!ctx) return 0;
    const int m = (int)ctx->impl->dtw_ran;
    ctx->impl->dtw_ran = 0;
    return m;
}

const char *rp_ctx_last_mlp_kernel(rp_ctx *ctx) { return ctx ? ctx->impl->last_mlp_kernel.c_str() : ""; }

size_t rp_mfcc_num_frames(size_t n_samples) {
    size_t chunks = n_samples / 480;
    return chunks >= 1 ? 3 * chunks - 3 : 0;
}

// whole streams of n_samples samples, pcm_stride apart
static bool pcm_args_ok(rp_sample_format fmt, size_t n_samples, size_t pcm_stride) {
    if (pcm_stride < n_samples) { set_last_error("pcm_stride smaller than n_samples"); return false; }
    return sample_format_ok(fmt);
}
static int widest_layer(const Model &m) {
    int maxd = 0;
    for (int d : m.dims) maxd = std::max(maxd, d);
    return maxd;
}

// The front of whole-stream detection: checks the PCM arguments, stages the PCM in and det / n_det out and writes the MFCC frames of
// every stream to ws_mfcc (timed).  Windows are max_len frames long.
// (DetectFront: rp_capi.h -- rp_bank_calls.cpp shares this front)
extern "C++" bool rp::detect_front(Ctx *c, Staged &sg, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride, int K,
                                   int max_len, rp_batch_detection *det, int32_t *n_det, int max_det, DetectFront *f) {
    if (!pcm_args_ok(fmt, n_samples, pcm_stride)) return false;
    const MfccTablesDev *tb = c->tables_for(K);
    if (!tb) return false;
    f->nf = rp_mfcc_num_frames(n_samples);
    f->n_win = f->nf >= (size_t)max_len ? f->nf - max_len + 1 : 0;
    f->rows = S * f->n_win;
    const void *dp = sg.in(pcm, S * pcm_stride * sample_bytes(fmt), c->stage_in);
    f->dd = static_cast<BatchDetection *>(sg.out(det, S * (size_t)max_det * sizeof(BatchDetection), c->stage_out));
    f->dn = static_cast<int32_t *>(sg.out(n_det, S * sizeof(int32_t), c->stage_out2));
    if (S && (!dp || !f->dd || !f->dn)) return false;
    if (!c->ws_mfcc.reserve(S * f->nf * K * sizeof(float) + 64 * K * sizeof(float))) return false;  // slack: the list kernel's band reads past a row
    f->dm = c->ws_mfcc.as<float>();
    return timed(c, kKernelMfcc, "mfcc_kernel", [&] { return launch_mfcc_fmt(c->stream, *tb, dp, (int)fmt, S, n_samples, pcm_stride, 0, f->nf, f->nf, f->dm); });
}

// detect_scan (rp_capi.h) with launch_scan over one wakeword's agg / avg (ww == nullptr), else launch_scan_multi over `ww` (dcol: each
// detection's wakeword or label)
static bool detect_scan(Ctx *c, const rp_detector_config &cfg, const float *dm, size_t S, size_t nf, int K, const ScanConfig &sc,
                        const float *dg, const float *da, uint32_t *hot, const ScanWakewords *ww, BatchDetection *dd, int32_t *dcol,
                        int32_t *dn, int max_det) {
    return detect_scan(c, cfg, dm, S, nf, K, "scan_kernel", [&](const float *dv, float vm) {
        return ww ? launch_scan_multi(c->stream, *ww, dv, vm, S, nf, sc, dd, dcol, dn, max_det)
                  : launch_scan(c->stream, dg, da, dv, vm, S, nf, sc, dd, dn, max_det, hot);
    });
}

int rp_mfcc_batch_fmt(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                      int K, float *mfcc) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        if (!pcm_args_ok(fmt, n_samples, pcm_stride)) return -1;
        const MfccTablesDev *tb = c->tables_for(K);
        if (!tb) return -1;
        const size_t nf = rp_mfcc_num_frames(n_samples);
        Staged sg(c);
        const void *dp = sg.in(pcm, S * pcm_stride * sample_bytes(fmt), c->stage_in);
        float *dm = static_cast<float *>(sg.out(mfcc, S * nf * K * sizeof(float), c->stage_out));
        if ((S && nf) && (!dp || !dm)) return -1;
        if (!timed(c, kKernelMfcc, "mfcc_kernel", [&] { return launch_mfcc_fmt(c->stream, *tb, dp, (int)fmt, S, n_samples, pcm_stride, 0, nf, nf, dm); }))
            return -1;
        if (!sg.back(mfcc, dm, S * nf * K * sizeof(float)) || !sg.finish()) return -1;
        return 0;
    });
}

int rp_mfcc_batch(rp_ctx *ctx, const float *pcm, size_t S, size_t n_samples, size_t pcm_stride, int K, float *mfcc) {
    return rp_mfcc_batch_fmt(ctx, pcm, RP_SAMPLE_F32, S, n_samples, pcm_stride, K, mfcc);
}

int rp_wakeword_ref_build(rp_ctx *ctx, const char *name, const float *threshold, const float *avg_threshold, size_t n,
                          const char *const *sample_names, const uint8_t *const *wav_buffers, const size_t *wav_lens,
                          uint16_t mfcc_size, int rms_from_files, uint8_t **out_rpw, size_t *out_len) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        *out_rpw = nullptr; *out_len = 0;
        WakewordRefData r;
        if (!build_wakeword_ref(ctx->impl.get(), name, threshold, avg_threshold, n, sample_names, wav_buffers, wav_lens,
                                (int)mfcc_size, rms_from_files != 0, &r)) return -1;
        std::vector<uint8_t> bytes = serialize_wakeword_ref(r);
        uint8_t *p = static_cast<uint8_t *>(std::malloc(bytes.size()));
        if (!p) { set_last_error("out of host memory"); return -1; }
        std::memcpy(p, bytes.data(), bytes.size());
        *out_rpw = p; *out_len = bytes.size();
        return 0;
    });
}
void rp_buffer_free(uint8_t *buffer) { std::free(buffer); }

int rp_mfcc_average_batch(rp_ctx *ctx, size_t n_wakewords, int mfcc_size, const int32_t *counts, const int32_t *lens, const float *feats,
                          float *avg) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        if (n_wakewords && (!counts || !lens || !feats || !avg)) { set_last_error("null argument"); return -1; }
        return average_templates_batch(ctx->impl.get(), n_wakewords, mfcc_size, counts, lens, feats, avg) ? 0 : -1;
    });
}

int rp_wakeword_ref_build_batch(rp_ctx *ctx, size_t n_wakewords, const char *const *names, const float *thresholds,
                                const float *avg_thresholds, const size_t *counts, const char *const *sample_names,
                                const uint8_t *const *wav_buffers, const size_t *wav_lens, uint16_t mfcc_size, int rms_from_files,
                                uint8_t **out_rpw, size_t *out_lens) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        if (n_wakewords && (!names || !counts || !out_rpw || !out_lens)) { set_last_error("null argument"); return -1; }
        size_t total = 0;
        for (size_t w = 0; w < n_wakewords; ++w) { out_rpw[w] = nullptr; out_lens[w] = 0; total += counts[w]; }
        if (total && (!sample_names || !wav_buffers || !wav_lens)) { set_last_error("null argument"); return -1; }
        std::vector<WakewordRefData> refs;
        if (!build_wakeword_refs(ctx->impl.get(), n_wakewords, names, thresholds, avg_thresholds, counts, sample_names, wav_buffers, wav_lens,
                                 (int)mfcc_size, rms_from_files != 0, &refs)) return -1;
        const std::vector<std::vector<uint8_t>> bytes = serialize_wakeword_refs(refs);   // everything that can throw comes before the first buffer is handed out
        for (size_t w = 0; w < n_wakewords; ++w) {
            uint8_t *p = static_cast<uint8_t *>(std::malloc(bytes[w].size()));
            if (!p) {
                for (size_t v = 0; v < w; ++v) { std::free(out_rpw[v]); out_rpw[v] = nullptr; out_lens[v] = 0; }
                set_last_error("out of host memory");
                return -1;
            }
            std::memcpy(p, bytes[w].data(), bytes[w].size());
            out_rpw[w] = p; out_lens[w] = bytes[w].size();
        }
        return 0;
    });
}

int rp_wakeword_model_train(rp_ctx *ctx, const rp_train_options *options, size_t n_train, const char *const *train_names,
                            const uint8_t *const *train_wavs, const size_t *train_lens, size_t n_test,
                            const char *const *test_names, const uint8_t *const *test_wavs, const size_t *test_lens,
                            const uint8_t *prev_model, size_t prev_model_len, uint8_t **out_rpw, size_t *out_len,
                            float *final_loss, float *test_accuracy) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        *out_rpw = nullptr; *out_len = 0;
        WakewordModelData prev, m;
        bool has_prev = false;
        if (prev_model) {
            RpwKind kind; WakewordRefData ref; std::string err;
            if (!parse_rpw(prev_model, prev_model_len, &kind, &ref, &prev, &err)) { set_last_error(err); return -1; }
            if (kind != RpwKind::Model) { set_last_error("the file to train from is not a wakeword model"); return -1; }
            has_prev = true;
        }
        if (!train_wakeword_model(ctx->impl.get(), *options, n_train, train_names, train_wavs, train_lens, n_test, test_names, test_wavs,
                                  test_lens, has_prev ? &prev : nullptr, &m, final_loss, test_accuracy)) return -1;
        std::vector<uint8_t> bytes = serialize_wakeword_model(m);
        uint8_t *p = static_cast<uint8_t *>(std::malloc(bytes.size()));
        if (!p) { set_last_error("out of host memory"); return -1; }
        std::memcpy(p, bytes.data(), bytes.size());
        *out_rpw = p; *out_len = bytes.size();
        return 0;
    });
}

int rp_wakeword_model_train_batch(rp_ctx *ctx, const rp_train_options *options, size_t n_models, const uint64_t *seeds,
                                  const size_t *train_counts, const char *const *train_names, const uint8_t *const *train_wavs,
                                  const size_t *train_lens, const size_t *test_counts, const char *const *test_names,
                                  const uint8_t *const *test_wavs, const size_t *test_lens, const uint8_t *const *prev_models,
                                  const size_t *prev_model_lens, uint8_t **out_rpw, size_t *out_lens, float *final_loss, float *test_accuracy) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        if (n_models && (!options || !train_counts || !test_counts || !out_rpw || !out_lens || (prev_models && !prev_model_lens))) {
            set_last_error("null argument");
            return -1;
        }
        size_t n_train = 0, n_test = 0;
        for (size_t w = 0; w < n_models; ++w) { out_rpw[w] = nullptr; out_lens[w] = 0; n_train += train_counts[w]; n_test += test_counts[w]; }
        if ((n_train && (!train_names || !train_wavs || !train_lens)) || (n_test && (!test_names || !test_wavs || !test_lens))) {
            set_last_error("null argument");
            return -1;
        }
        std::vector<WakewordModelData> prev(prev_models ? n_models : 0), models;
        std::vector<const WakewordModelData *> prev_of(n_models, nullptr);
        for (size_t w = 0; prev_models && w < n_models; ++w) {
            if (!prev_models[w]) continue;
            RpwKind kind; WakewordRefData ref; std::string err;
            if (!parse_rpw(prev_models[w], prev_model_lens[w], &kind, &ref, &prev[w], &err)) { set_last_error("model " + std::to_string(w) + ": " + err); return -1; }
            if (kind != RpwKind::Model) { set_last_error("model " + std::to_string(w) + ": the file to train from is not a wakeword model"); return -1; }
            prev_of[w] = &prev[w];
        }
        if (!train_wakeword_models(ctx->impl.get(), *options, n_models, seeds, train_counts, train_names, train_wavs, train_lens, test_counts,
                                   test_names, test_wavs, test_lens, prev_of.data(), &models, final_loss, test_accuracy)) return -1;
        std::vector<std::vector<uint8_t>> bytes(n_models);   // everything that can throw comes before the first buffer is handed out
        parallel_for(n_models, [&](size_t w) { bytes[w] = serialize_wakeword_model(models[w]); });
        for (size_t w = 0; w < n_models; ++w) {
            uint8_t *p = static_cast<uint8_t *>(std::malloc(bytes[w].size()));
            if (!p) {
                for (size_t v = 0; v < w; ++v) { std::free(out_rpw[v]); out_rpw[v] = nullptr; out_lens[v] = 0; }
                set_last_error("out of host memory");
                return -1;
            }
            std::memcpy(p, bytes[w].data(), bytes[w].size());
            out_rpw[w] = p; out_lens[w] = bytes[w].size();
        }
        return 0;
    });
}

int rp_mlp_train_batch(rp_ctx *ctx, size_t n_models, const int32_t *n_layers, const int32_t *dims, const int32_t *n_rows, const float *x,
                       const int32_t *labels, float *params, float learning_rate, size_t epochs, float *final_loss) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        if (n_models && (!n_layers || !dims || !n_rows || !x || !labels || !params)) { set_last_error("null argument"); return -1; }
        ctx->impl->train_feature_ms = 0.0;
        std::vector<MlpTrainItem> items(n_models);
        std::vector<std::vector<float>> loss_rows(n_models);
        size_t x_at = 0, row_at = 0, param_at = 0;
        for (size_t w = 0; w < n_models; ++w) {
            MlpTrainItem &it = items[w];
            const std::string who = "model " + std::to_string(w) + ": ";
            if (n_layers[w] < 1 || n_layers[w] > kTrainMaxLayers) { set_last_error(who + "an MLP of 1 to 4 layers is required"); return -1; }
            if (n_rows[w] < 1) { set_last_error(who + "no rows to train on"); return -1; }
            it.n_layers = n_layers[w];
            for (int l = 0; l <= it.n_layers; ++l) {
                it.dims[l] = dims[w * (kTrainMaxLayers + 1) + l];
                if (it.dims[l] < 1) { set_last_error(who + "layer widths must be >= 1"); return -1; }
            }
            it.B = (size_t)n_rows[w];
            it.x = x + x_at; it.labels = labels + row_at; it.params = params + param_at;
            loss_rows[w].assign(it.B, 0.f);
            it.loss_rows = loss_rows[w].data();
            x_at += it.B * (size_t)it.dims[0]; row_at += it.B;
            for (int l = 0; l < it.n_layers; ++l) param_at += ((size_t)it.dims[l] + 1) * (size_t)it.dims[l + 1];
        }
        if (!train_mlp_batch(ctx->impl.get(), items, learning_rate, epochs)) return -1;
        for (size_t w = 0; final_loss && w < n_models; ++w) {   // the mean over the rows, summed in order (train_wakeword_model)
            float s = 0.f;
            for (float v : loss_rows[w]) s += v;
            final_loss[w] = epochs ? s / (float)items[w].B : NAN;
        }
        return 0;
    });
}

int rp_train_batch_last_profile(rp_ctx *ctx, double *feature_ms, double *longest_launch_ms, int *launches) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    const Ctx *c = ctx->impl.get();
    if (feature_ms) *feature_ms = c->train_feature_ms;
    if (longest_launch_ms) *longest_launch_ms = c->train_longest_launch_ms;
    if (launches) *launches = c->train_launches;
    return 0;
}

int rp_frontend_batch(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                      const rp_filters_config *filters, float rms_level_ref, size_t window_size, float *pcm_out,
                      size_t out_stride, float *rms, float *gains) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        return frontend_batch(ctx->impl.get(), pcm, fmt, S, n_samples, pcm_stride, filters, rms_level_ref, window_size, nullptr, nullptr, pcm_out,
                              out_stride, rms, gains);
    });
}

int rp_templates_new(rp_ctx *ctx, int T, int K, const int *lens, const float *feats, int avg_len, const float *avg,
                     rp_templates **out) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        *out = nullptr;
        std::unique_ptr<Templates> t(Templates::create(ctx->impl.get(), T, K, lens, feats, avg_len, avg));
        if (!t) return -1;
        rp_templates *h = new rp_templates();
        h->impl = std::move(t);
        *out = h;
        return 0;
    });
}
void rp_templates_free(rp_templates *t) { delete t; }
int rp_templates_max_len(const rp_templates *t) { return t ? t->impl->dev.max_len : 0; }

int rp_dtw_score_batch(rp_ctx *ctx, const float *mfcc, size_t S, size_t n_frames, const rp_templates *t,
                       float score_ref, int band_size, rp_score_mode score_mode, int with_avg, float *scores,
                       float *avg, float *agg) {
    return guarded([&]() -> int {
        if (!ctx || !t) { set_last_error("null handle"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        const TemplatesDev &td = t->impl->dev;
        if (n_frames < (size_t)td.max_len) return 0;  // no complete window
        if (band_size < 0) { set_last_error("band_size must be >= 0"); return -1; }  // 0: no cell is in the band, every score is 0 (dtw.rs:64-75)
        const size_t n_win = n_frames - td.max_len + 1;
        const bool do_avg = with_avg && td.has_avg;
        if (do_avg && !avg) { set_last_error("avg output required when with_avg is set"); return -1; }
        Staged sg(c);
        const size_t rows = S * n_win;
        const float *dm = static_cast<const float *>(sg.in(mfcc, S * n_frames * td.K * sizeof(float), c->stage_in));
        float *ds = static_cast<float *>(sg.out(scores, rows * td.T * sizeof(float), c->stage_out));
        float *da = do_avg ? static_cast<float *>(sg.out(avg, rows * sizeof(float), c->stage_out2)) : nullptr;
        float *dg = agg ? static_cast<float *>(sg.out(agg, rows * sizeof(float), c->stage_out3)) : nullptr;
        if (rows && (!dm || !ds)) return -1;
        DtwScore q;
        q.t = &td; q.mfcc = dm; q.S = S; q.frame_pitch = n_frames; q.n_win = n_win; q.band = band_size; q.score_ref = score_ref;
        q.with_avg = do_avg; q.score_mode = (int)score_mode; q.scores = ds; q.avg = da; q.agg = dg;
        q.ragged = true; q.padded_rows = false;
        if (!dtw_score(*c, q)) return -1;
        if (!sg.back(scores, ds, rows * td.T * sizeof(float)) || (do_avg && !sg.back(avg, da, rows * sizeof(float))) ||
            (dg && !sg.back(agg, dg, rows * sizeof(float))) || !sg.finish())
            return -1;
        return 0;
    });
}

int rp_detect_scan(rp_ctx *ctx, const float *agg, const float *avg, size_t S, size_t n_frames, int max_len,
                   const rp_detector_config *config, int avg_enabled, const float *mfcc, int K,
                   rp_batch_detection *det, int32_t *n_det, int max_det) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        if (!config || (S && (!agg || !det || !n_det))) { set_last_error("null argument"); return -1; }
        // a window of no frames would give every stream n_frames + 1 rows: more than the caller's agg / avg hold
        if (max_len < 1) { set_last_error("rp_detect_scan: max_len must be >= 1"); return -1; }
        if (max_det < 0) { set_last_error("rp_detect_scan: max_det must be >= 0"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        const bool vad = config->vad_mode != RP_VAD_NONE;
        if (vad && (!mfcc || K < 1)) { set_last_error("rp_detect_scan: vad_mode needs the MFCC frames"); return -1; }
        static_assert(sizeof(rp_batch_detection) == sizeof(BatchDetection), "layout");
        const ScanConfig sc = scan_config(*config, max_len, avg_enabled && avg);
        const size_t n_win = n_frames >= (size_t)max_len ? n_frames - max_len + 1 : 0;
        Staged sg(c);
        const float *dg = static_cast<const float *>(sg.in(agg, S * n_win * sizeof(float), c->stage_in));
        const float *da = sc.avg_enabled ? static_cast<const float *>(sg.in(avg, S * n_win * sizeof(float), c->stage_out3)) : nullptr;
        BatchDetection *dd = static_cast<BatchDetection *>(sg.out(det, S * (size_t)max_det * sizeof(BatchDetection), c->stage_out));
        int32_t *dn = static_cast<int32_t *>(sg.out(n_det, S * sizeof(int32_t), c->stage_out2));
        const float *dm = vad ? static_cast<const float *>(sg.in(mfcc, S * n_frames * K * sizeof(float), c->ws_mfcc)) : nullptr;
        if (vad && S * n_frames && !dm) return -1;
        if (!detect_scan(c, *config, dm, S, n_frames, K, sc, dg, da, nullptr, nullptr, dd, nullptr, dn, max_det)) return -1;
        return sg.back_detections(S, max_det, det, dd, n_det, dn) && sg.finish() ? 0 : -1;
    });
}

int rp_batch_detect(rp_ctx *ctx, const float *pcm, size_t S, size_t n_samples, size_t pcm_stride, const rp_templates *t,
                    const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det, int max_det,
                    float *scores, float *agg) {
    return rp_batch_detect_fmt(ctx, pcm, RP_SAMPLE_F32, S, n_samples, pcm_stride, t, config, det, n_det, max_det, scores, agg);
}

// The body of rp_batch_detect_fmt.  gather (rp_batch_detect_sharded): the detections of this shard are reported with
// stream ids starting at stream_base and, instead of going to `det` / `n_det` directly, are copied from this context's
// buffers into the gathered block `det` / `n_det` (rows stream_base..) that lives in host memory (gather_host) or on
// device gather_device (peer copy over xGMI).
struct GatherTo { bool on = false, host = true; int device = 0; int stream_base = 0; bool device_pcm = false; };   // device_pcm: pcm is a device pointer whatever the context's flags say (rp_batch_detect_ingest)
static int batch_detect_impl(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                             const rp_templates *t, const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det,
                             int max_det, float *scores, float *agg, const GatherTo &gather) {
    return guarded([&]() -> int {
        if (!ctx || !t) { set_last_error("null handle"); return -1; }
        if (!config || (S && (!pcm || !det || !n_det))) { set_last_error("null argument"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        const TemplatesDev &td = t->impl->dev;
        const bool do_avg = td.has_avg && config->avg_threshold != 0.f;  // wakeword_comp.rs:85
        Staged sg(c);
        if (gather.device_pcm) sg.host = false;
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, td.K, td.max_len, det, n_det, max_det, &f)) return -1;
        const size_t nf = f.nf, n_win = f.n_win, rows = f.rows;
        if (gather.on) {  // results are produced in this context's own buffers and copied into the gathered block below
            if (!c->stage_out.reserve(S * (size_t)max_det * sizeof(BatchDetection) + 16) || !c->stage_out2.reserve(S * sizeof(int32_t) + 16)) return -1;
            f.dd = c->stage_out.as<BatchDetection>(); f.dn = c->stage_out2.as<int32_t>();
        }
        // caller-provided score arrays are used directly when they are device pointers
        float *ds = (scores && !sg.host) ? scores : nullptr, *dg = (agg && !sg.host) ? agg : nullptr;
        c->last_window_scores = 0;
        if (!ds) { if (!c->ws_scores.reserve(rows * td.T * sizeof(float) + 16)) return -1; ds = c->ws_scores.as<float>(); }
        const bool ds_is_ws = ds == c->ws_scores.as<float>();
        if (!dg) { if (!c->ws_agg.reserve(rows * sizeof(float) + 16)) return -1; dg = c->ws_agg.as<float>(); }
        float *da = nullptr;
        if (do_avg) { if (!c->ws_avg.reserve(rows * sizeof(float) + 16)) return -1; da = c->ws_avg.as<float>(); }
        // ws_mfcc ends with slack (padded rows): short streams (fewer than 64 windows each) are scored by cross-stream waves like
        // live-stream batches.  The averaged-template gate is taken when the caller did not ask for the per-window score arrays (those
        // are defined for every window) and RP_CTX_FULL_SCORES is not set.
        DtwScore q;
        q.t = &td; q.mfcc = f.dm; q.S = S; q.frame_pitch = nf; q.n_win = n_win; q.band = config->band_size; q.score_ref = config->score_ref;
        q.with_avg = do_avg; q.detect_only = !scores && !agg && !(c->flags & RP_CTX_FULL_SCORES);
        q.avg_threshold = config->avg_threshold; q.threshold = config->threshold; q.score_mode = (int)config->score_mode;
        q.scores = ds; q.avg = da; q.agg = dg;
        q.gate_generic = true; q.fuse_max = true; q.ragged = true;
        if (n_win) {   // the aggregate pass also tells the scan which streams can fire at all (a flag per stream)
            q.hot = c->hot_flags(S);   // zero: the scan below puts every flag it reads back (no memset per call)
            if (!q.hot) return -1;
        }
        if (!dtw_score(*c, q)) return -1;
        if (ds_is_ws) c->last_window_scores = rows * (size_t)td.T;   // rp_ctx_last_window_scores
        ScanConfig sc = scan_config(*config, td.max_len, do_avg);
        sc.stream_base = gather.stream_base;
        if (!detect_scan(c, *config, f.dm, S, nf, td.K, sc, dg, da, q.hot, nullptr, f.dd, nullptr, f.dn, max_det)) return -1;
        if (gather.on) {
            // final result gather: this shard's block into the gathered arrays -- device to host, or a peer
            // copy to the gathering device (xGMI between the GPUs of a node)
            rp_batch_detection *gd = det + (size_t)gather.stream_base * (size_t)max_det;
            int32_t *gn = n_det + gather.stream_base;
            const size_t bd = S * (size_t)max_det * sizeof(BatchDetection), bn = S * sizeof(int32_t);
            if (gather.host) {
                if (!hip_ok(hipMemcpyAsync(gd, f.dd, bd, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(gather)") ||
                    !hip_ok(hipMemcpyAsync(gn, f.dn, bn, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(gather)")) return -1;
            } else {
                if (!hip_ok(hipMemcpyPeerAsync(gd, gather.device, f.dd, c->device, bd, c->stream), "hipMemcpyPeerAsync(gather)") ||
                    !hip_ok(hipMemcpyPeerAsync(gn, gather.device, f.dn, c->device, bn, c->stream), "hipMemcpyPeerAsync(gather)")) return -1;
            }
            return hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize") ? 0 : -1;
        }
        if (!sg.back_detections(S, max_det, det, f.dd, n_det, f.dn)) return -1;
        if (sg.host && scores && !sg.back(scores, ds, rows * td.T * sizeof(float))) return -1;
        if (sg.host && agg && !sg.back(agg, dg, rows * sizeof(float))) return -1;
        return sg.finish() ? 0 : -1;
    });
}

int rp_batch_detect_fmt(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                        const rp_templates *t, const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det,
                        int max_det, float *scores, float *agg) {
    return batch_detect_impl(ctx, pcm, fmt, S, n_samples, pcm_stride, t, config, det, n_det, max_det, scores, agg, GatherTo{});
}

// how the last rp_batch_detect_sharded of this thread gathered its results (rp_sharded_gather_info)
static thread_local std::string g_sharded_info;
const char *rp_sharded_gather_info(void) { return g_sharded_info.c_str(); }

int rp_batch_detect_ingest(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                           const rp_templates *t, const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det,
                           int max_det, size_t block_streams, double *seconds) {
    return guarded([&]() -> int {
        if (!ctx || !t) { set_last_error("null handle"); return -1; }
        if (!config || (S && (!pcm || !det || !n_det))) { set_last_error("null argument"); return -1; }
        if (!sample_format_ok(fmt)) return -1;
        if (pcm_stride < n_samples) { set_last_error("pcm_stride smaller than n_samples"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        const auto t0 = std::chrono::steady_clock::now();
        const size_t Sb = block_streams ? block_streams : 8192, row_bytes = pcm_stride * sample_bytes(fmt);
        const size_t blk = std::min(Sb, S), n_blocks = S ? (S + blk - 1) / blk : 0;
        if (S > 0x7fffffffULL) { set_last_error("rp_batch_detect_ingest: too many streams"); return -1; }
        if (n_blocks == 0) { if (seconds) *seconds = 0.0; return 0; }
        if (!c->ingest_ready() || !c->ws_ingest.reserve(2 * blk * row_bytes + 64)) return -1;
        unsigned char *dbuf[2] = {c->ws_ingest.as<unsigned char>(), c->ws_ingest.as<unsigned char>() + blk * row_bytes};
        auto streams_of = [&](size_t k) { return std::min(blk, S - k * blk); };
        auto copy_block = [&](size_t k) {   // on the copy stream, once the kernels that last read this buffer are done
            const int b = (int)(k & 1);
            return hip_ok(hipStreamWaitEvent(c->copy_stream, c->ingest_freed[b], 0), "hipStreamWaitEvent") &&
                   hip_ok(hipMemcpyAsync(dbuf[b], static_cast<const unsigned char *>(pcm) + k * blk * row_bytes, streams_of(k) * row_bytes,
                                         hipMemcpyHostToDevice, c->copy_stream), "hipMemcpyAsync(ingest)") &&
                   hip_ok(hipEventRecord(c->ingest_landed[b], c->copy_stream), "hipEventRecord");
        };
        // every way out after the first copy was queued waits for the copy stream: a copy from the caller's buffer may still be in flight,
        // and the caller is free to release or reuse `pcm` the moment this call returns -- error or not
        auto fail = [&]() {
            const std::string why = last_error();
            (void)hipStreamSynchronize(c->copy_stream);
            (void)hipGetLastError();
            set_last_error(why);
            return -1;
        };
        for (int b = 0; b < 2; ++b)
            if (!hip_ok(hipEventRecord(c->ingest_freed[b], c->stream), "hipEventRecord")) return -1;
        if (!copy_block(0)) return fail();
        for (size_t k = 0; k < n_blocks; ++k) {
            const int b = (int)(k & 1);
            if (k + 1 < n_blocks && !copy_block(k + 1)) return fail();   // the next block's copy goes out before this block's kernels
            if (!hip_ok(hipStreamWaitEvent(c->stream, c->ingest_landed[b], 0), "hipStreamWaitEvent")) return fail();
            GatherTo g;
            g.on = true; g.host = true; g.stream_base = (int)(k * blk); g.device_pcm = true;
            // the block through the ordinary batched path; its detections land in det / n_det at the block's rows (the call waits for them)
            if (batch_detect_impl(ctx, dbuf[b], fmt, streams_of(k), n_samples, pcm_stride, t, config, det, n_det, max_det, nullptr, nullptr, g) != 0) return fail();
            if (!hip_ok(hipEventRecord(c->ingest_freed[b], c->stream), "hipEventRecord")) return fail();
        }
        if (!hip_ok(hipStreamSynchronize(c->copy_stream), "hipStreamSynchronize")) return -1;
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    });
}

int rp_batch_detect_sharded(rp_ctx *const *ctxs, const rp_templates *const *t, int n_shards, const void *const *pcm,
                            rp_sample_format fmt, const size_t *S, size_t n_samples, size_t pcm_stride,
                            const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det, int max_det) {
    return guarded([&]() -> int {
        if (!ctxs || !t || !pcm || !S || !config || !det || !n_det) { set_last_error("null argument"); return -1; }
        if (n_shards < 1 || n_shards > 64) { set_last_error("rp_batch_detect_sharded: 1..64 shards"); return -1; }
        size_t total = 0;
        std::vector<size_t> first((size_t)n_shards);
        for (int g = 0; g < n_shards; ++g) {
            if (!ctxs[g] || !t[g]) { set_last_error("null handle"); return -1; }
            if (t[g]->impl->ctx != ctxs[g]->impl.get()) { set_last_error("rp_batch_detect_sharded: templates[g] must have been created on ctxs[g]"); return -1; }
            if ((ctxs[g]->impl->flags & RP_CTX_HOST_POINTERS) != (ctxs[0]->impl->flags & RP_CTX_HOST_POINTERS)) {
                set_last_error("rp_batch_detect_sharded: all contexts must agree on RP_CTX_HOST_POINTERS"); return -1;
            }
            for (int h = 0; h < g; ++h) if (ctxs[h] == ctxs[g]) { set_last_error("rp_batch_detect_sharded: a context may serve one shard only"); return -1; }
            if (S[g] && !pcm[g]) { set_last_error("null argument"); return -1; }
            first[g] = total; total += S[g];
        }
        if (total > 0x7fffffffULL) { set_last_error("rp_batch_detect_sharded: too many streams"); return -1; }
        GatherTo to;
        to.on = true; to.host = (ctxs[0]->impl->flags & RP_CTX_HOST_POINTERS) != 0; to.device = ctxs[0]->impl->device;
        // one host thread per shard drives that shard's device and stream; the shards share nothing but read-only inputs
        std::vector<int> status((size_t)n_shards, 0);
        std::vector<std::string> errs((size_t)n_shards);
        // device-resident gather: let every other device write into ctxs[0]'s device directly (xGMI) where the node allows it;
        // without peer access hipMemcpyPeerAsync still works (staged by the runtime), so a refusal here is not an error
        std::string info = to.host ? "gather into host memory (RP_CTX_HOST_POINTERS): device-to-host copies" : "gather onto device " + std::to_string(to.device) + ":";
        if (!to.host)
            for (int g = 1; g < n_shards; ++g) {
                const int dev = ctxs[g]->impl->device;
                int can = 0;
                const char *how = dev == to.device ? "same device" : "staged by the runtime (no peer access)";
                if (dev != to.device && hipDeviceCanAccessPeer(&can, dev, to.device) == hipSuccess && can && hipSetDevice(dev) == hipSuccess) {
                    const hipError_t pe = hipDeviceEnablePeerAccess(to.device, 0);
                    if (pe == hipSuccess) how = "peer access enabled (direct write over xGMI)";
                    else if (pe == hipErrorPeerAccessAlreadyEnabled) how = "peer access already enabled (direct write over xGMI)";
                    else how = "staged by the runtime (hipDeviceEnablePeerAccess refused)";
                    if (pe != hipSuccess) (void)hipGetLastError();  // hipErrorPeerAccessAlreadyEnabled or a refusal: both fine
                }
                info += " shard " + std::to_string(g) + " (device " + std::to_string(dev) + "): " + how + ";";
            }
        g_sharded_info = info;
        auto run = [&](int g) noexcept {
            try {
                GatherTo mine = to;
                mine.stream_base = (int)first[g];
                status[g] = S[g] ? batch_detect_impl(ctxs[g], pcm[g], fmt, S[g], n_samples, pcm_stride, t[g], config, det, n_det, max_det, nullptr,
                                                     nullptr, mine) : 0;
                if (status[g] != 0) errs[g] = last_error();  // the error text is thread-local: hand it to the caller's thread
            } catch (...) {  // e.g. bad_alloc while copying the error text: never let an exception leave a thread
                status[g] = -1;
            }
        };
        // shard 0 runs on the caller's thread; if the process cannot start another thread the remaining shards run here too
        std::vector<std::thread> th;
        th.reserve((size_t)n_shards);
        int on_threads = 1;  // shards [1, on_threads) have a thread of their own
        for (int g = 1; g < n_shards; ++g) {
            try { th.emplace_back(run, g); } catch (const std::system_error &) { break; }
            on_threads = g + 1;
        }
        run(0);
        for (int g = on_threads; g < n_shards; ++g) run(g);
        for (auto &x : th) x.join();
        for (int g = 0; g < n_shards; ++g)
            if (status[g] != 0) { set_last_error("shard " + std::to_string(g) + ": " + (errs[g].empty() ? std::string("failed") : errs[g])); return -1; }
        return 0;
    });
}

int rp_batch_detect_multi(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                          size_t n_wakewords, const rp_templates *const *t, const rp_detector_config *config,
                          const float *thresholds, const float *avg_thresholds, rp_batch_detection *det,
                          int32_t *det_wakeword, int32_t *n_det, int max_det) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        if (!config || !t || (S && (!pcm || !det || !n_det))) { set_last_error("null argument"); return -1; }
        for (size_t j = 0; j < n_wakewords && j < (size_t)kScanMaxWakewords; ++j) if (!t[j]) { set_last_error("null handle"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        if (n_wakewords < 1 || n_wakewords > (size_t)kScanMaxWakewords) { set_last_error("rp_batch_detect_multi: 1..8 wakewords"); return -1; }
        const int K = t[0]->impl->dev.K;
        int max_len = 0;
        size_t maxT = 1;
        for (size_t j = 0; j < n_wakewords; ++j) {
            const TemplatesDev &td = t[j]->impl->dev;
            if (td.K != K) { set_last_error("Usage of wakewords with different mfcc size is not supported, ignoring wakeword"); return -1; }
            max_len = std::max(max_len, td.max_len);  // on_wakeword_change, src/detector.rs:328-334: max over the wakewords' frame sizes
            maxT = std::max<size_t>(maxT, (size_t)td.T);
        }
        Staged sg(c);
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, K, max_len, det, n_det, max_det, &f)) return -1;
        const size_t nf = f.nf, n_win = f.n_win, rows = f.rows;
        int32_t *dw = det_wakeword ? static_cast<int32_t *>(sg.out(det_wakeword, S * (size_t)max_det * sizeof(int32_t), c->stage_out3)) : nullptr;
        ScanWakewords ww{};
        ww.n = (int)n_wakewords;
        // one shared per-template score buffer, per wakeword its aggregate / avg rows
        if (!c->ws_scores.reserve(rows * maxT * sizeof(float) + 16) || !c->ws_agg.reserve(n_wakewords * rows * sizeof(float) + 16) ||
            !c->ws_avg.reserve(n_wakewords * rows * sizeof(float) + 16)) return -1;
        float *ds = c->ws_scores.as<float>();
        c->last_window_scores = 0;   // the wakewords share the buffer: no [S * n_win][T] block of one call is left in it
        for (size_t j = 0; j < n_wakewords; ++j) {
            const TemplatesDev &td = t[j]->impl->dev;
            const float thr = thresholds && !std::isnan(thresholds[j]) ? thresholds[j] : config->threshold;
            const float athr = avg_thresholds && !std::isnan(avg_thresholds[j]) ? avg_thresholds[j] : config->avg_threshold;
            const bool do_avg = td.has_avg && athr != 0.f;  // wakeword_comp.rs:85
            float *dg = c->ws_agg.as<float>() + j * rows, *da = do_avg ? c->ws_avg.as<float>() + j * rows : nullptr;
            if (n_win) {
                DtwScore q;
                q.t = &td; q.mfcc = f.dm; q.S = S; q.frame_pitch = nf; q.n_win = n_win; q.band = config->band_size; q.score_ref = config->score_ref;
                q.with_avg = do_avg; q.detect_only = !(c->flags & RP_CTX_FULL_SCORES);   // this entry point has no per-window outputs
                q.avg_threshold = athr; q.threshold = thr; q.score_mode = (int)config->score_mode;
                q.scores = ds; q.avg = da; q.agg = dg;
                if (!dtw_score(*c, q)) return -1;
            }
            ww.agg[j] = dg; ww.avg[j] = da; ww.threshold[j] = thr; ww.avg_threshold[j] = athr;
        }
        if (!detect_scan(c, *config, f.dm, S, nf, K, scan_config(*config, max_len, false), nullptr, nullptr, nullptr, &ww, f.dd, dw, f.dn, max_det))
            return -1;
        return sg.back_detections(S, max_det, det, f.dd, n_det, f.dn, det_wakeword, dw) && sg.finish() ? 0 : -1;
    });
}

int rp_resampler_frame_lengths(size_t sample_rate, size_t *in_len, size_t *out_len) {
    return guarded([&]() -> int {
        if (!in_len || !out_len) { set_last_error("null argument"); return -1; }
        if (!resampler_frame_lengths(sample_rate, in_len, out_len)) {
            set_last_error("Unsupported sample rate, unable to initialize the resampler");
            return -1;
        }
        return 0;
    });
}

int rp_resample_batch(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, int channels, size_t sample_rate, size_t S,
                      size_t n_samples, size_t pcm_stride, float *out, size_t out_stride) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        if (!sample_format_ok(fmt)) return -1;
        if (channels < 1) { set_last_error("Unsupported channel count"); return -1; }
        if (pcm_stride < n_samples * (size_t)channels) { set_last_error("pcm_stride smaller than n_samples * channels"); return -1; }
        const Resampler *rs = c->resampler_for(sample_rate);
        if (!rs) return -1;
        const size_t n_chunks = n_samples / (size_t)rs->dev.fi, n_out = n_chunks * (size_t)rs->dev.fo;
        if (out_stride < n_out) { set_last_error("out_stride smaller than the resampled length"); return -1; }
        if (S == 0 || n_chunks == 0) return 0;
        Staged sg(c);
        const void *dp = sg.in(pcm, S * pcm_stride * sample_bytes(fmt), c->stage_in);
        float *dout = static_cast<float *>(sg.out(out, S * out_stride * sizeof(float), c->stage_out));
        if (!dp || !dout) return -1;
        if (!resample_rows(c, rs->dev, dp, (int)fmt, channels, pcm_stride, nullptr, nullptr, S, n_chunks, c->ws_resample, n_chunks, dout, out_stride)) return -1;
        if (!sg.back(out, dout, S * out_stride * sizeof(float)) || !sg.finish()) return -1;
        return 0;
    });
}

int rp_model_new(rp_ctx *ctx, int n_layers, const int *dims, const float *const *weights, const float *const *biases,
                 rp_model **out) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        *out = nullptr;
        std::unique_ptr<Model> m(Model::create(ctx->impl.get(), n_layers, dims, weights, biases));
        if (!m) return -1;
        rp_model *h = new rp_model();
        h->impl = std::move(m);
        *out = h;
        return 0;
    });
}
void rp_model_free(rp_model *m) { delete m; }

int rp_mlp_forward_batch(rp_ctx *ctx, const rp_model *model, const float *x, size_t B, int precision, float *logits) {
    return guarded([&]() -> int {
        if (!ctx || !model) { set_last_error("null handle"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        Model &m = *model->impl;
        const int nl = (int)m.dims.size() - 1;
        if (!mlp_precision_ok(precision)) return -1;
        Staged sg(c);
        const float *dx = static_cast<const float *>(sg.in(x, B * (size_t)m.dims[0] * 4, c->stage_in));
        float *dl = static_cast<float *>(sg.out(logits, B * (size_t)m.dims[nl] * 4, c->stage_out));
        if (B && (!dx || !dl)) return -1;
        MlpForward q;
        q.m = &m; q.precision = precision; q.x = dx; q.B = B; q.out = dl;
        if (!m.mfma_ok) {
            if (precision == RP_MLP_BF16) { set_last_error("this layer-1 shape has no bf16 MFMA kernel"); return -1; }
            const int maxd = widest_layer(m);
            if (!c->stage_out2.reserve(B * (size_t)maxd * 4) || !c->stage_out3.reserve(B * (size_t)maxd * 4)) return -1;
            q.scratch[0] = c->stage_out2.as<float>(); q.scratch[1] = c->stage_out3.as<float>();
        }
        if (!mlp_forward(*c, q)) return -1;
        if (!sg.back(logits, dl, B * (size_t)m.dims[nl] * 4) || !sg.finish()) return -1;
        return 0;
    });
}

int rp_mlp_forward_windows(rp_ctx *ctx, const rp_model *model, const float *mfcc, size_t S, size_t n_frames, int mfcc_size, int precision,
                           float *logits) {
    return guarded([&]() -> int {
        if (!ctx || !model) { set_last_error("null handle"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        Model &m = *model->impl;
        const int nl = (int)m.dims.size() - 1, K = mfcc_size;
        if (!mlp_precision_ok(precision)) return -1;
        if (K < 1 || m.dims[0] % K != 0) { set_last_error("Model input size does not match the mfcc size"); return -1; }
        const int L = m.dims[0] / K;
        const size_t n_win = n_frames >= (size_t)L ? n_frames - L + 1 : 0, rows = S * n_win;
        if (rows == 0) return 0;
        if (!mfcc || !logits) { set_last_error("null argument"); return -1; }
        Staged sg(c);
        const float *dm = static_cast<const float *>(sg.in(mfcc, S * n_frames * (size_t)K * 4, c->stage_in));
        float *dl = static_cast<float *>(sg.out(logits, rows * (size_t)m.dims[nl] * 4, c->stage_out));
        if (!dm || !dl) return -1;
        c->last_window_scores = 0;   // ws_scores serves the forward here
        if (!window_logits(c, m, dm, S, n_frames, n_win, L, K, precision, dl, c->ws_gain, c->ws_scores, c->ws_gain, false)) return -1;
        if (!sg.back(logits, dl, rows * (size_t)m.dims[nl] * 4) || !sg.finish()) return -1;
        return 0;
    });
}

int rp_batch_detect_model(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                          const rp_model *model, int mfcc_size, int none_index, const rp_detector_config *config, int precision,
                          rp_batch_detection *det, int32_t *det_label, int32_t *n_det, int max_det) {
    return guarded([&]() -> int {
        if (!ctx || !model) { set_last_error("null handle"); return -1; }
        if (!config || (S && (!pcm || !det || !n_det))) { set_last_error("null argument"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        if (!mlp_precision_ok(precision)) return -1;
        Model &m = *model->impl;
        const int K = mfcc_size;
        if (K < 1 || m.dims[0] % K != 0) { set_last_error("Incorrect model layers"); return -1; }
        const int L = m.dims[0] / K, n_labels = m.dims.back();
        if (none_index >= n_labels) { set_last_error("none_index out of range"); return -1; }
        if (!m.mfma_ok && precision == RP_MLP_BF16) { set_last_error("this layer-1 shape has no bf16 MFMA kernel"); return -1; }
        Staged sg(c);
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, K, L, det, n_det, max_det, &f)) return -1;
        const size_t nf = f.nf, n_win = f.n_win, rows = f.rows;
        int32_t *dl = det_label ? static_cast<int32_t *>(sg.out(det_label, S * (size_t)max_det * sizeof(int32_t), c->stage_out3)) : nullptr;
        if (!c->ws_ring.reserve(rows * (size_t)n_labels * sizeof(float) + 16) || !c->ws_agg.reserve(rows * sizeof(float) + 16) ||
            !c->ws_avg.reserve(rows * sizeof(float) + 16) || !c->ws_rms.reserve(rows * sizeof(int32_t) + 16)) return -1;
        float *dlog = c->ws_ring.as<float>();
        c->last_window_scores = 0;   // ws_scores serves the forward here
        if (!window_logits(c, m, f.dm, S, nf, n_win, L, K, precision, dlog, c->ws_gain, c->ws_scores, c->ws_gain, false)) return -1;
        float *dg = c->ws_agg.as<float>(), *da = c->ws_avg.as<float>();
        int32_t *dlab = c->ws_rms.as<int32_t>();
        // nn_score_kernel also tells the scan which streams have a window that passed (a flag per stream, like the aggregate pass of
        // the reference path): the others are not swept
        uint32_t *hot = nullptr;
        if (n_win) {
            hot = c->hot_flags(S);
            if (!hot) return -1;
        }
        if (!hip_ok(launch_nn_score(c->stream, dlog, rows, n_labels, none_index, config->score_ref * 10.f, config->avg_threshold != 0.f ? 1 : 0,
                                    config->threshold, config->avg_threshold, dg, da, dlab, hot, n_win), "nn_score_kernel")) return -1;
        ScanWakewords ww{};
        ww.n = 1; ww.agg[0] = dg; ww.avg[0] = da; ww.label[0] = dlab; ww.hot = hot;
        ww.threshold[0] = -1.f; ww.avg_threshold[0] = -1.f;  // the gates were applied by nn_score_kernel (>=, not >)
        if (!detect_scan(c, *config, f.dm, S, nf, K, scan_config(*config, L, false), nullptr, nullptr, nullptr, &ww, f.dd, dl, f.dn, max_det))
            return -1;
        return sg.back_detections(S, max_det, det, f.dd, n_det, f.dn, det_label, dl) && sg.finish() ? 0 : -1;
    });
}

int rp_synth_pcm_batch(rp_ctx *ctx, uint64_t seed, uint64_t first_stream, size_t S, size_t n_samples, size_t pcm_stride,
                       float *pcm) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        Staged sg(c);
        float *dp = static_cast<float *>(sg.out(pcm, S * pcm_stride * sizeof(float), c->stage_out));
        if (S && n_samples && !dp) return -1;
        if (!hip_ok(launch_synth(c->stream, seed, first_stream, S, n_samples, pcm_stride, dp), "synth_kernel")) return -1;
        if (!sg.back(pcm, dp, S * pcm_stride * sizeof(float)) || !sg.finish()) return -1;
        return 0;
    });
}

int rp_ctx_timing_enable(rp_ctx *ctx, int enable) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    ctx->impl->timing = enable != 0;
    return 0;
}
int rp_ctx_timing_reset(rp_ctx *ctx) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    ctx->impl->time_collect();
    for (int i = 0; i < kKernelCount; ++i) { ctx->impl->sum_ms[i] = 0; ctx->impl->count[i] = 0; }
    return 0;
}
int rp_ctx_timing_read(rp_ctx *ctx, int kernel, double *avg_ms, int *launches) {
    if (!ctx) { set_last_error("null handle"); return -1; }
    if (kernel < 0 || kernel >= kKernelCount) { set_last_error("unknown kernel id"); return -1; }
    ctx->impl->time_collect();
    int n = ctx->impl->count[kernel];
    if (avg_ms) *avg_ms = n ? ctx->impl->sum_ms[kernel] / n : 0.0;
    if (launches) *launches = n;
    return 0;
}

}  // extern "C"

// BandPassFilter::new, band_pass_filter.rs:31-55 (f32, sample rate 16 kHz): q = a0 a1 a2 b1 b2, zeros when the filter is off
void rp::band_pass_coefficients(const rp_band_pass_config &b, float q[5]) {
    float a0 = 0, a1 = 0, a2 = 0, b1 = 0, b2 = 0;
    if (b.enabled) {
        const float kPi = 3.14159274101257324f, sample_rate = 16000.f;
        const float omega_low = 2.0f * kPi * b.low_cutoff / sample_rate, omega_high = 2.0f * kPi * b.high_cutoff / sample_rate;
        const float cos_low = std::cos(omega_low), cos_high = std::cos(omega_high);
        const float alpha_low = std::sin(omega_low) / 2.0f, alpha_high = std::sin(omega_high) / 2.0f;
        a0 = 1.0f / (1.0f + alpha_high - alpha_low);
        a1 = -2.0f * cos_low * a0; a2 = (1.0f - alpha_high - alpha_low) * a0;
        b1 = -2.0f * cos_high * a0; b2 = (1.0f - alpha_high + alpha_low) * a0;
    }
    q[0] = a0; q[1] = a1; q[2] = a2; q[3] = b1; q[4] = b2;
}

// Logits of every window of L frames of S streams' MFCC rows (WakewordNN::run_detection's forward, window by window,
// src/wakewords/nn/wakeword_nn.rs:101-159): dlog [S * n_win][labels].  Window w of stream s starts at frame s * pitch + w from `first`.
// The workspaces: `mean` for the window means of the in-place form, `xrows` for the normalised rows and `scratch` for the per-layer kernel.
// live (live-stream batches): all rows in one slab, so a call makes one launch, and rp_ctx_last_mlp_kernel is left as it is by the
// in-place form.  Shared by rp_batch_detect_model, rp_mlp_forward_windows and the live batches' model wakewords.
bool rp::window_logits(Ctx *c, Model &m, const float *first, size_t S, size_t pitch, size_t n_win, int L, int K, int precision,
                       float *dlog, DevBuf &mean, DevBuf &xrows, DevBuf &scratch, bool live) {
    const size_t rows = S * n_win;
    const int n_labels = m.dims.back();
    MlpForward q;
    q.m = &m; q.precision = precision;
    // windows read in place from the frame array, the window mean taken out after layer 1
    q.wsum = (m.mfma_ok && K % 4 == 0) ? m.wsum_for(K) : nullptr;
    if (q.wsum) {
        if (!mean.reserve(rows * (size_t)K * sizeof(float) + 16)) return false;
        if (!hip_ok(launch_window_means(c->stream, first, S, pitch, n_win, L, K, mean.as<float>()), "window_means_kernel")) return false;
        q.windows = true; q.x = first; q.S = S; q.n_win = n_win; q.frame_pitch = pitch; q.K = K; q.mean = mean.as<float>(); q.out = dlog;
        q.report = !live;
        return mlp_forward(*c, q);
    }
    // windows are materialised slab by slab (a row is dims[0] floats): <= 4 GiB of rows at a time
    const size_t row_bytes = (size_t)m.dims[0] * sizeof(float);
    const size_t slab = live ? rows : std::min(rows, std::max<size_t>(1, ((size_t)4 << 30) / row_bytes));
    const int maxd = widest_layer(m);
    if (!xrows.reserve(slab * row_bytes + 64)) return false;
    if (!m.mfma_ok) {
        if (!scratch.reserve(2 * slab * (size_t)maxd * sizeof(float) + 16)) return false;
        q.scratch[0] = scratch.as<float>(); q.scratch[1] = scratch.as<float>() + slab * (size_t)maxd;
    }
    q.x = xrows.as<float>();
    for (size_t r0 = 0; r0 < rows; r0 += slab) {
        q.B = std::min(slab, rows - r0);
        q.out = dlog + r0 * n_labels;
        if (!hip_ok(launch_normalize_windows_batch(c->stream, first, pitch, n_win, r0, q.B, L, K, xrows.as<float>()), "normalize_windows_kernel") ||
            !mlp_forward(*c, q))
            return false;
    }
    return true;
}

// S rows of n_chunks input frames -> 16 kHz rows `out` (rp_resample_batch, the live batches' encode stage): read where they lie when the
// FFT kernel can, else staged into xs_buf, reserved here for xs_chunks frames a row.  prev / prev_out (live streams; nullptr = silence
// before the rows): every stream's previous input frame, and where the last frame of this call is kept for the next.
bool rp::resample_rows(Ctx *c, const ResamplerDev &rs, const void *pcm, int fmt, int channels, size_t pcm_stride, const float *prev,
                       float *prev_out, size_t S, size_t n_chunks, DevBuf &xs_buf, size_t xs_chunks, float *out, size_t out_stride) {
    if (resample_reads_in_place(rs, pcm, fmt, pcm_stride, out, out_stride))
        return timed(c, kKernelResample, "resample48_fft_kernel", [&] {
            return launch_resample_in_place(c->stream, rs, pcm, fmt, channels, pcm_stride, prev, prev_out, S, n_chunks, out, out_stride); });
    const size_t fi = (size_t)rs.fi;
    if (!xs_buf.reserve(S * (1 + xs_chunks) * fi * sizeof(float) + 64)) return false;
    float *xs = xs_buf.as<float>();
    return hip_ok(launch_resample_stage(c->stream, pcm, fmt, channels, S, n_chunks, rs.fi, pcm_stride, prev, xs), "resample_stage_kernel") &&
           timed(c, kKernelResample, "resample kernel", [&] { return launch_resample(c->stream, rs, xs, S, n_chunks, out, out_stride); }) &&
           (!prev_out || hip_ok(launch_carry_rows(c->stream, xs, S, (1 + n_chunks) * fi, n_chunks * fi, fi, prev_out, fi), "carry_rows_kernel"));
}
