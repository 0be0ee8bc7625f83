// rp_capi.h -- what the files of the extern "C" surface share (rp_capi.cpp, rp_bank.cpp, rp_bank_calls.cpp, rp_model_bank.cpp, rp_stream_batch.cpp).  Not installed.
#pragma once
#include <new>

#include "rp_host.h"

struct rp_ctx { std::unique_ptr<rp::Ctx> impl; };
struct rp_templates { std::unique_ptr<rp::Templates> impl; };
struct rp_model { std::unique_ptr<rp::Model> impl; };
struct rp_wakeword_bank { std::unique_ptr<rp::Bank> impl; };
struct rp_model_bank { std::unique_ptr<rp::ModelBank> impl; };

namespace rp {

template <class F> int guarded(F &&f) {
    try { return f(); }
    catch (const std::bad_alloc &) { set_last_error("out of host memory"); return -1; }
    catch (const std::exception &e) { set_last_error(e.what()); return -1; }
    catch (...) { set_last_error("unknown error"); return -1; }
}

// one launch, timed as `kernel` when the context times its kernels (rp_ctx_timing_enable)
template <class F> bool timed(Ctx *c, int kernel, const char *what, F &&launch) {
    c->time_begin(kernel);
    const bool ok = hip_ok(launch(), what);
    c->time_end();
    return ok;
}

struct Staged {  // host<->device staging for RP_CTX_HOST_POINTERS
    Ctx *c;
    bool host;
    explicit Staged(Ctx *ctx) : c(ctx), host((ctx->flags & RP_CTX_HOST_POINTERS) != 0) {}
    const void *in(const void *p, size_t bytes, DevBuf &buf) {
        if (!host || !p) return p;
        if (!buf.reserve(bytes)) return nullptr;
        if (!hip_ok(hipMemcpyAsync(buf.p, p, bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(H2D)")) return nullptr;
        return buf.p;
    }
    void *out(void *p, size_t bytes, DevBuf &buf) {
        if (!host || !p) return p;
        return buf.reserve(bytes) ? buf.p : nullptr;
    }
    bool back(void *host_p, const void *dev_p, size_t bytes) {
        if (!host || !host_p) return true;
        return hip_ok(hipMemcpyAsync(host_p, dev_p, bytes, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync(D2H)");
    }
    bool finish() { return !host || hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize"); }
    // det [S][max_det] and n_det [S], then the int32 column per detection `col` (det_wakeword / det_label) when there is one
    bool back_detections(size_t S, int max_det, rp_batch_detection *det, const BatchDetection *dd, int32_t *n_det, const int32_t *dn,
                         int32_t *col = nullptr, const int32_t *dcol = nullptr) {
        return back(det, dd, S * (size_t)max_det * sizeof(BatchDetection)) && back(n_det, dn, S * sizeof(int32_t)) &&
               (!dcol || back(col, dcol, S * (size_t)max_det * sizeof(int32_t)));
    }
};

inline size_t sample_bytes(rp_sample_format f) { return f == RP_SAMPLE_I8 ? 1 : f == RP_SAMPLE_I16 ? 2 : 4; }
inline float vad_mode_value(rp_vad_mode m) { return m == RP_VAD_EASY ? 2.f : m == RP_VAD_MEDIUM ? 2.5f : 3.f; }  // src/config.rs:140-146

inline bool sample_format_ok(rp_sample_format fmt) {
    if ((int)fmt < 0 || (int)fmt > 3) { set_last_error("unknown sample format"); return false; }
    return true;
}
inline bool mlp_precision_ok(int p) {
    if (p != RP_MLP_F32 && p != RP_MLP_BF16 && p != RP_MLP_F32_STRICT && p != RP_MLP_F32_FAST) { set_last_error("unknown MLP precision"); return false; }
    return true;
}

// fpf 0: the ScanConfig default (whole streams, 30 ms frames)
inline ScanConfig scan_config(const rp_detector_config &cfg, int max_len, bool avg_enabled, int fpf = 0) {
    ScanConfig sc;
    sc.threshold = cfg.threshold; sc.avg_threshold = cfg.avg_threshold; sc.min_scores = (int)cfg.min_scores;
    sc.eager = cfg.eager ? 1 : 0; sc.max_len = max_len; sc.avg_enabled = avg_enabled ? 1 : 0;
    if (fpf) sc.fpf = fpf;
    return sc;
}

// rp_capi.cpp
// whole-stream detection after detect_front: device det / n_det, the MFCC frames ws_mfcc [S][nf][K], windows per stream
struct DetectFront {
    BatchDetection *dd = nullptr;
    int32_t *dn = nullptr;
    float *dm = nullptr;
    size_t nf = 0, n_win = 0, rows = 0;
};
bool detect_front(Ctx *c, Staged &sg, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride, int K,
                  int max_len, rp_batch_detection *det, int32_t *n_det, int max_det, DetectFront *f);
bool window_logits(Ctx *c, Model &m, const float *first, size_t S, size_t pitch, size_t n_win, int L, int K, int precision,
                   float *dlog, DevBuf &mean, DevBuf &xrows, DevBuf &scratch, bool live);
void band_pass_coefficients(const rp_band_pass_config &b, float q[5]);
bool resample_rows(Ctx *c, const ResamplerDev &rs, const void *pcm, int fmt, int channels, size_t pcm_stride, const float *prev,
                   float *prev_out, size_t S, size_t n_chunks, DevBuf &xs_buf, size_t xs_chunks, float *out, size_t out_stride);
// The tail of whole-stream detection: VAD values of the frames dm [S][nf][K] when vad_mode is on (dv, else null), then the timed scan
// launch(dv, vad_mode_value); `what` names the scan kernel in an error
template <class F> bool detect_scan(Ctx *c, const rp_detector_config &cfg, const float *dm, size_t S, size_t nf, int K, const char *what, F &&launch) {
    float *dv = nullptr;
    if (cfg.vad_mode != RP_VAD_NONE) {
        if (!c->ws_vad.reserve(S * nf * sizeof(float) + 16)) return false;
        dv = c->ws_vad.as<float>();
        if (!hip_ok(launch_vad_value(c->stream, dm, S * nf, K, dv), "vad_value_kernel")) return false;
    }
    const float vm = vad_mode_value(cfg.vad_mode);
    return timed(c, kKernelScan, what, [&] { return launch(dv, vm); });
}
// rp_bank.cpp
bool bank_band_ok(const Bank &bk, int band_size);
bool set_size_ok(int set_size);   // within 1 .. RP_WAKEWORD_SET_MAX
// rp_bank_calls.cpp
bool model_set_size_ok(int set_size);   // within 1 .. RP_MODEL_SET_MAX
// after the null-handle test of a call over a bank: the bank's owner must be the call's context, whose device becomes current; null with the error set
inline Ctx *bank_call_ctx(rp_ctx *ctx, const Ctx *owner) {
    Ctx *c = ctx->impl.get();
    if (owner != c) { set_last_error("the bank belongs to another context"); return nullptr; }
    return hip_ok(hipSetDevice(c->device), "hipSetDevice") ? c : nullptr;
}
// Bank indices of n streams in a HOST array, idx [n] (set_size 0) or [n][set_size]: every one within [-1, W), else an error that names stream
// first + i (and the slot) and the index, `what` being "wakeword index" or "model index"
bool bank_indices_ok(int W, size_t first, size_t n, int set_size, const int32_t *idx, const char *what = "wakeword index");
// The per-stream indices of a whole-recording call.  Host arrays are checked before anything is launched and copied to ws_bank_idx;
// max_n_win is the window count of the longest window a stream of the call has (sets: of its longest live slot).  Device arrays are taken
// as they are: the kernels treat an index outside [0, W) as "none", and max_n_win is the window count of the bank's shortest window.
// S == 0 succeeds with dev null.
struct BankIndices {
    const int32_t *dev = nullptr;
    size_t max_n_win = 0;
};
bool stage_bank_indices(Ctx *c, Staged &sg, const Bank &bk, const int32_t *idx, size_t S, int set_size, size_t n_frames, BankIndices *bi);
// rp_frontend_batch and rp_frontend_batch_bank (rp_capi.cpp): with `bank`, every stream takes its gain window and reference level from its own
// wakeword bank[stream_wakeword[s]] and rms_level_ref / window_size are not read.  With `sides` (rp_frontend_batch_bank_sets / _model_bank /
// _mixed_sets; `bank` and stream_wakeword null): sides[0] / sides[1] are the DEVICE rows [S][set_size] the caller staged and checked with
// their banks -- one bank: the second side absent; mixed sets: references, then models -- window_size is the capacity of a stream's ring
// (the largest window of the banks the rows index), and every stream's level and window come from stream_targets_kernel.
int frontend_batch(Ctx *c, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride, const rp_filters_config *filters,
                   float rms_level_ref, size_t window_size, const Bank *bank, const int32_t *stream_wakeword, float *pcm_out, size_t out_stride,
                   float *rms, float *gains, const TargetSide *sides = nullptr);

}  // namespace rp
