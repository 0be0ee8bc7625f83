// rp_bank_calls.cpp -- the whole-recording calls over a bank.  Stream s is scored against ITS wakeword of a wakeword bank (rp_dtw_score_bank,
// rp_batch_detect_bank, rp_frontend_batch_bank; kernels: rp_dtw_bank.hip, scan_bank_kernel in rp_scan.hip), against its own SET of wakewords
// (rp_dtw_score_bank_sets, rp_batch_detect_bank_sets; rp_dtw_set.hip, rp_scan_sets.hip), or is run by ITS model of a model bank
// (rp_mlp_forward_windows_bank, rp_batch_detect_model_bank; mlp_windows_bank_kernel, window_means_bank_kernel, nn_score_bank_kernel in
// rp_mlp_windows.hip / rp_mlp.hip), or holds references of a wakeword bank AND models of a model bank on one detector (mixed sets:
// rp_batch_detect_mixed_sets, rp_frontend_batch_mixed_sets; rp_gain_targets.hip, scan_mixed_set_kernel in rp_scan_sets.hip).  Every call
// reads: arguments, staged indices, the empty-bank answer, front, score, scan, copy back.  The banks themselves are rp_bank.cpp and
// rp_model_bank.cpp; DESIGN.md sections 4.2 - 4.4.
#include <algorithm>
#include <cstring>
#include <initializer_list>

#include "rp_capi.h"

using namespace rp;

namespace rp {

bool bank_indices_ok(int W, size_t first, size_t n, int set_size, const int32_t *idx, const char *what) {
    const size_t row = set_size ? (size_t)set_size : 1;
    for (size_t i = 0; i < n * row; ++i)
        if (idx[i] < -1 || idx[i] >= W) {
            set_last_error("stream " + std::to_string(first + i / row) + (set_size ? ", slot " + std::to_string(i % row) : std::string()) + ": " + what +
                           " " + std::to_string(idx[i]) + " is outside the bank (-1 .. " + std::to_string(W - 1) + ")");
            return false;
        }
    return true;
}

// The indices of a call over any bank of W entries, idx [S] (set_size 0) or [S][set_size].  min_len: the bank's shortest window; len_of(w):
// the window of entry w; used (optional, [W]): set for every entry a stream of a HOST array uses.
template <class LenOf>
static bool stage_indices(Ctx *c, Staged &sg, int W, int min_len, LenOf len_of, const char *what, const int32_t *idx, size_t S, int set_size,
                          size_t n_frames, BankIndices *bi, std::vector<char> *used = nullptr, DevBuf *buf = nullptr) {
    auto n_win_of = [&](int len) { return n_frames >= (size_t)len ? n_frames - (size_t)len + 1 : (size_t)0; };
    *bi = BankIndices();
    if (!sg.host) {
        if (W > 0) bi->max_n_win = n_win_of(min_len);
        bi->dev = idx;
        return true;
    }
    if (!bank_indices_ok(W, 0, S, set_size, idx, what)) return false;
    const size_t row = set_size ? (size_t)set_size : 1;
    for (size_t s = 0; s < S; ++s) {
        int lmax = 0;   // the stream's window: that of its longest live slot
        for (size_t j = 0; j < row; ++j) {
            const int32_t wi = idx[s * row + j];
            if (wi < 0) continue;
            lmax = std::max(lmax, len_of((size_t)wi));
            if (used) (*used)[(size_t)wi] = 1;
        }
        if (lmax > 0) bi->max_n_win = std::max(bi->max_n_win, n_win_of(lmax));
    }
    if (S == 0) return true;
    bi->dev = static_cast<const int32_t *>(sg.in(idx, S * row * sizeof(int32_t), buf ? *buf : c->ws_bank_idx));   // (buf: a call that stages two arrays)
    return bi->dev != nullptr;
}

bool stage_bank_indices(Ctx *c, Staged &sg, const Bank &bk, const int32_t *idx, size_t S, int set_size, size_t n_frames, BankIndices *bi) {
    return stage_indices(c, sg, bk.dev.W, bk.dev.min_len, [&](size_t w) { return bk.ww[w].max_len; }, "wakeword index", idx, S, set_size, n_frames, bi);
}

bool model_set_size_ok(int set_size) {
    if (set_size < 1 || set_size > RP_MODEL_SET_MAX) {
        set_last_error("set_size " + std::to_string(set_size) + " is outside 1 .. " + std::to_string((int)RP_MODEL_SET_MAX) + " (RP_MODEL_SET_MAX)");
        return false;
    }
    return true;
}

}  // namespace rp

namespace {

// The indices of a call over a model bank and its launch shape: that of the models the call's streams use (host arrays), of every model of
// the bank (device arrays)
struct ModelBankCall {
    BankIndices idx;
    ModelBankShape shape;
};
bool stage_model_indices(Ctx *c, Staged &sg, const ModelBank &bk, const int32_t *idx, size_t S, size_t n_frames, ModelBankCall *q) {
    std::vector<char> used(bk.e.size(), sg.host ? 0 : 1);
    if (!stage_indices(c, sg, bk.dev.W, bk.min_L, [&](size_t w) { return bk.e[w].L; }, "model index", idx, S, 0, n_frames, &q->idx, &used)) return false;
    for (size_t w = 0; w < bk.e.size(); ++w)
        if (used[w]) model_bank_shape_add(&q->shape, n_frames, bk.e[w].L, bk.e[w].tail_floats);
    return true;
}

// The same for rows of set_size indices (model sets): Lmax(s), the longest window of a row's live slots, decides the stream's window count
// and cut, every live slot's own window the staging -- host arrays: of the rows as they are; device arrays: of every pair the bank allows
bool stage_model_set_indices(Ctx *c, Staged &sg, const ModelBank &bk, const int32_t *idx, size_t S, int set_size, size_t n_frames, ModelBankCall *q,
                             DevBuf *buf = nullptr) {
    if (!stage_indices(c, sg, bk.dev.W, bk.min_L, [&](size_t w) { return bk.e[w].L; }, "model index", idx, S, set_size, n_frames, &q->idx, nullptr, buf)) return false;
    if (sg.host) {
        for (size_t s = 0; s < S; ++s) {
            const int32_t *row = idx + s * (size_t)set_size;
            int lmax = 0;
            for (int j = 0; j < set_size; ++j) if (row[j] >= 0) lmax = std::max(lmax, bk.e[(size_t)row[j]].L);
            for (int j = 0; j < set_size; ++j)
                if (row[j] >= 0) model_set_shape_add(&q->shape, n_frames, lmax, bk.e[(size_t)row[j]].L, bk.e[(size_t)row[j]].tail_floats);
        }
        return true;
    }
    std::vector<char> is_len(257, 0);   // a bank's windows are at most 256 frames
    for (const ModelBankEntry &e : bk.e) if (e.L >= 1 && e.L <= 256) is_len[(size_t)e.L] = 1;
    for (int lmax = 1; lmax <= 256; ++lmax)
        if (is_len[(size_t)lmax])
            for (const ModelBankEntry &e : bk.e) model_set_shape_add(&q->shape, n_frames, lmax, e.L, e.tail_floats);
    return true;
}

// tail: the reference-bank calls end the refusal "... of the call (N)", the model-bank call "... of the call, N"; both are public behaviour
bool pitch_ok(size_t win_pitch, size_t max_n_win, bool model = false) {
    if (win_pitch >= max_n_win) return true;
    const std::string n = std::to_string(max_n_win);
    set_last_error("win_pitch " + std::to_string(win_pitch) + " is smaller than the largest window count of the call" + (model ? ", " + n : " (" + n + ")"));
    return false;
}

// A Rustpotter without wakewords: the PCM arguments and max_det are checked as the front would check them, no stream reports anything and
// every row is zero (the bank's mfcc_size is a placeholder).  more: det_wakeword / det_label and the score rows, where the call has them.
struct ZeroOut { void *p; size_t bytes; };
int empty_bank_answer(Ctx *c, Staged &sg, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride, rp_batch_detection *det, int32_t *n_det,
                      int max_det, std::initializer_list<ZeroOut> more) {
    if (!sample_format_ok(fmt)) return -1;
    if (pcm_stride < n_samples) { set_last_error("pcm_stride smaller than n_samples"); return -1; }
    if (max_det < 0) { set_last_error("max_det must be >= 0"); return -1; }
    auto zero = [&](void *p, size_t bytes) {
        if (!p || !bytes) return true;
        if (sg.host) { std::memset(p, 0, bytes); return true; }
        return hip_ok(hipMemsetAsync(p, 0, bytes, c->stream), "hipMemsetAsync");
    };
    if (!zero(det, S * (size_t)max_det * sizeof(rp_batch_detection)) || !zero(n_det, S * sizeof(int32_t))) return -1;
    for (const ZeroOut &z : more) if (!zero(z.p, z.bytes)) return -1;
    return sg.finish() ? 0 : -1;
}

// score rows of a detect call: the caller's array when it is a device pointer, else the workspace (host pointers: Staged::back copies it back)
float *out_rows(Staged &sg, float *user, size_t bytes, DevBuf &ws) {
    if (user && !sg.host) return user;
    return ws.reserve(bytes + 16) ? ws.as<float>() : nullptr;
}

// the timed launch (kernel 1 of rp_ctx_timing_read); band_size 0: no cell lies in the band and every score is 0 (dtw.rs:64-75); an empty
// bank: no stream has a wakeword, every row is zero
bool score_bank(Ctx *c, const Bank &bk, BankScore &q) {
    if (q.S == 0 || q.win_pitch == 0) return true;
    if (q.band == 0 || bk.dev.W == 0) {
        if (!hip_ok(hipMemsetAsync(q.agg, 0, q.S * q.win_pitch * sizeof(float), c->stream), "hipMemsetAsync")) return false;
        return !q.avg || hip_ok(hipMemsetAsync(q.avg, 0, q.S * q.win_pitch * sizeof(float), c->stream), "hipMemsetAsync");
    }
    const DtwWork wk = c->dtw_work();
    q.fix = wk.fix;
    dtw_mark(wk, kDtwRanBank);
    return timed(c, kKernelDtw, "dtw_bank_kernel", [&] { return launch_dtw_bank(c->stream, bk.dev, q); });
}

// the same for a call over sets (dtw_set_kernel); zero rows for band_size 0 and an empty bank, proposals "nobody" (-1)
bool score_bank_sets(Ctx *c, const Bank &bk, BankSetScore &q) {
    if (q.S == 0 || q.win_pitch == 0) return true;
    if (q.band == 0 || bk.dev.W == 0) {
        const size_t row = q.S * q.win_pitch * sizeof(float), slots = row * (size_t)q.set_size;
        auto fill = [&](void *p, int v, size_t bytes) { return !p || hip_ok(hipMemsetAsync(p, v, bytes, c->stream), "hipMemsetAsync"); };
        return fill(q.best, 0, row) && fill(q.best_avg, 0, row) && fill(q.best_ww, 0xff, row) && fill(q.slot_agg, 0, slots) && fill(q.slot_avg, 0, slots);
    }
    const DtwWork wk = c->dtw_work();
    q.fix = wk.fix;
    dtw_mark(wk, kDtwRanBankSets);
    return timed(c, kKernelDtw, "dtw_set_kernel", [&] { return launch_dtw_set(c->stream, bk.dev, q); });
}

// RP_MLP_F32, or RP_MLP_BF16 computed as RP_MLP_F32 (as rp_mlp_forward_windows); the forms with a second pass over listed rows or with
// the f32 matrix instructions are not built for a bank
bool bank_precision_ok(int precision) {
    if (!mlp_precision_ok(precision)) return false;
    if (precision == RP_MLP_F32_FAST || precision == RP_MLP_F32_STRICT) {
        set_last_error("model bank calls take RP_MLP_F32 (three bf16 parts; RP_MLP_BF16 computes the same): RP_MLP_F32_FAST and RP_MLP_F32_STRICT are not built for a bank");
        return false;
    }
    return true;
}

// window means, then the forward inside the context's kKernelMlp bracket: dlog [S][pitch][label_pitch]
bool bank_logits(Ctx *c, const ModelBank &bk, const ModelBankCall &q, const float *dm, size_t S, size_t nf, size_t pitch, float *dlog) {
    if (!c->ws_gain.reserve(S * pitch * 16 * sizeof(float) + 16)) return false;
    float *mean = c->ws_gain.as<float>();
    if (!hip_ok(launch_window_means_bank(c->stream, bk.dev, q.idx.dev, dm, S, nf, pitch, mean), "window_means_bank_kernel")) return false;
    if (!timed(c, kKernelMlp, "mlp_windows_bank_kernel", [&] { return launch_mlp_windows_bank(c->stream, bk.dev, q.shape, q.idx.dev, dm, S, nf, mean, pitch, dlog); }))
        return false;
    c->last_mlp_kernel = "mlp_windows_bank_kernel<bf16x3 splits>";
    return true;
}

// the same over the rows (s, j) of a call over model sets: dlog [S][set_size][pitch][label_pitch], one forward launch
bool bank_set_logits(Ctx *c, const ModelBank &bk, const ModelBankCall &q, int set_size, const float *dm, size_t S, size_t nf, size_t pitch, float *dlog) {
    if (!c->ws_gain.reserve(S * (size_t)set_size * pitch * 16 * sizeof(float) + 16)) return false;
    float *mean = c->ws_gain.as<float>();
    if (!hip_ok(launch_window_means_model_set(c->stream, bk.dev, q.idx.dev, set_size, dm, S, nf, pitch, mean), "window_means_model_set_kernel")) return false;
    if (!timed(c, kKernelMlp, "mlp_windows_model_set_kernel", [&] {
            return launch_mlp_windows_model_set(c->stream, bk.dev, q.shape, q.idx.dev, set_size, dm, S, nf, mean, pitch, dlog); }))
        return false;
    c->last_mlp_kernel = "mlp_windows_model_set_kernel<bf16x3 splits>";
    return true;
}

}  // namespace

extern "C" {

int rp_dtw_score_bank(rp_ctx *ctx, const float *mfcc, size_t S, size_t n_frames, const rp_wakeword_bank *bank, const int32_t *stream_wakeword,
                      float score_ref, int band_size, rp_score_mode score_mode, int with_avg, float *avg, float *agg, size_t win_pitch) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (S && (!mfcc || !stream_wakeword || !agg)) { set_last_error("null argument"); return -1; }
        const Bank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_band_ok(bk, band_size)) return -1;
        Staged sg(c);
        BankIndices bi;
        if (!stage_bank_indices(c, sg, bk, stream_wakeword, S, 0, n_frames, &bi) || !pitch_ok(win_pitch, bi.max_n_win)) return -1;
        if (S == 0 || win_pitch == 0) return sg.finish() ? 0 : -1;   // (the indices may be on their way to the device)
        const size_t out_bytes = S * win_pitch * sizeof(float);
        BankScore q;
        q.mfcc = static_cast<const float *>(sg.in(mfcc, S * n_frames * bk.dev.K * sizeof(float), c->stage_in));
        q.agg = static_cast<float *>(sg.out(agg, out_bytes, c->stage_out3));
        q.avg = avg ? static_cast<float *>(sg.out(avg, out_bytes, c->stage_out2)) : nullptr;
        if ((n_frames && !q.mfcc) || !q.agg || (avg && !q.avg)) return -1;
        q.S = S; q.n_frames = n_frames; q.win_pitch = win_pitch; q.stream_wakeword = bi.dev; q.band = band_size; q.score_mode = (int)score_mode;
        q.score_ref = score_ref; q.avg_mode = with_avg ? 1 : 0;
        if (!score_bank(c, bk, q)) return -1;
        return sg.back(agg, q.agg, out_bytes) && sg.back(avg, q.avg, out_bytes) && sg.finish() ? 0 : -1;
    });
}

int rp_dtw_score_bank_sets(rp_ctx *ctx, const float *mfcc, size_t S, size_t n_frames, const rp_wakeword_bank *bank, const int32_t *stream_wakewords,
                           int set_size, float score_ref, int band_size, rp_score_mode score_mode, int with_avg, float *avg, float *agg, size_t win_pitch) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!set_size_ok(set_size)) return -1;
        if (S && (!mfcc || !stream_wakewords || !agg)) { set_last_error("null argument"); return -1; }
        const Bank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_band_ok(bk, band_size)) return -1;
        Staged sg(c);
        BankIndices bi;
        if (!stage_bank_indices(c, sg, bk, stream_wakewords, S, set_size, n_frames, &bi) || !pitch_ok(win_pitch, bi.max_n_win)) return -1;
        if (S == 0 || win_pitch == 0) return sg.finish() ? 0 : -1;
        const size_t out_bytes = S * (size_t)set_size * win_pitch * sizeof(float);
        BankSetScore q;
        q.mfcc = static_cast<const float *>(sg.in(mfcc, S * n_frames * bk.dev.K * sizeof(float), c->stage_in));
        q.slot_agg = static_cast<float *>(sg.out(agg, out_bytes, c->stage_out3));
        q.slot_avg = avg ? static_cast<float *>(sg.out(avg, out_bytes, c->stage_out2)) : nullptr;
        if ((n_frames && !q.mfcc) || !q.slot_agg || (avg && !q.slot_avg)) return -1;
        q.S = S; q.n_frames = n_frames; q.win_pitch = win_pitch; q.stream_wakewords = bi.dev; q.set_size = set_size; q.band = band_size;
        q.score_mode = (int)score_mode; q.score_ref = score_ref; q.avg_mode = with_avg ? 1 : 0;
        if (!score_bank_sets(c, bk, q)) return -1;
        return sg.back(agg, q.slot_agg, out_bytes) && sg.back(avg, q.slot_avg, out_bytes) && sg.finish() ? 0 : -1;
    });
}

// rp_frontend_batch with every stream's own gain window and reference level (gain_per_stream_kernel); the chunk RMS and apply kernels are
// those of rp_frontend_batch -- they take per-chunk gains
int rp_frontend_batch_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                           const rp_filters_config *filters, const rp_wakeword_bank *bank, const int32_t *stream_wakeword,
                           float *pcm_out, size_t out_stride, float *rms, float *gains) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (S && !stream_wakeword) { set_last_error("null argument"); return -1; }
        if (bank->impl->ctx != ctx->impl.get()) { set_last_error("the bank belongs to another context"); return -1; }
        return frontend_batch(ctx->impl.get(), pcm, fmt, S, n_samples, pcm_stride, filters, 0.f, 0, bank->impl.get(), stream_wakeword, pcm_out,
                              out_stride, rms, gains);
    });
}

// ... with every stream's SET of wakewords: the level and window of on_wakeword_change (src/detector.rs:328-338) per stream, prepared by
// stream_targets_kernel in front of the same kernels.  Indices as rp_dtw_score_bank_sets takes them.
int rp_frontend_batch_bank_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                const rp_filters_config *filters, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int set_size,
                                float *pcm_out, size_t out_stride, float *rms, float *gains) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (S && !stream_wakewords) { set_last_error("null argument"); return -1; }
        if (!set_size_ok(set_size)) return -1;
        const Bank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c) return -1;
        Staged sg(c);
        BankIndices bi;   // a refused index: before anything is launched or written
        if (!stage_bank_indices(c, sg, bk, stream_wakewords, S, set_size, 0, &bi)) return -1;
        const TargetSide sides[2] = {{bi.dev, set_size, bk.dev.ww, bk.rms_level, bk.dev.W}, {}};
        return frontend_batch(c, pcm, fmt, S, n_samples, pcm_stride, filters, 0.f, (size_t)std::max(bk.dev.max_len / 3, 1), nullptr, nullptr, pcm_out,
                              out_stride, rms, gains, sides);
    });
}

// ... with every stream's model, or set of models, of a model bank (set_size 1: rp_batch_detect_model_bank's streams)
int rp_frontend_batch_model_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                 const rp_filters_config *filters, const rp_model_bank *bank, const int32_t *stream_models, int set_size,
                                 float *pcm_out, size_t out_stride, float *rms, float *gains) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (S && !stream_models) { set_last_error("null argument"); return -1; }
        if (!model_set_size_ok(set_size)) return -1;
        const ModelBank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c) return -1;
        Staged sg(c);
        BankIndices bi;
        if (!stage_indices(c, sg, bk.dev.W, bk.min_L, [&](size_t w) { return bk.e[w].L; }, "model index", stream_models, S, set_size, 0, &bi)) return -1;
        const TargetSide sides[2] = {{bi.dev, set_size, bk.scan.ww, bk.rms_level(), bk.dev.W}, {}};
        return frontend_batch(c, pcm, fmt, S, n_samples, pcm_stride, filters, 0.f, (size_t)std::max(bk.max_L / 3, 1), nullptr, nullptr, pcm_out,
                              out_stride, rms, gains, sides);
    });
}

int rp_batch_detect_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                         const rp_wakeword_bank *bank, const int32_t *stream_wakeword, const rp_detector_config *config,
                         rp_batch_detection *det, int32_t *n_det, int max_det, float *agg, float *avg, size_t win_pitch) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!config || (S && (!pcm || !stream_wakeword || !det || !n_det))) { set_last_error("null argument"); return -1; }
        const Bank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_band_ok(bk, (int)config->band_size)) return -1;
        Staged sg(c);
        const size_t nf = rp_mfcc_num_frames(n_samples);
        BankIndices bi;
        if (!stage_bank_indices(c, sg, bk, stream_wakeword, S, 0, nf, &bi)) return -1;
        const bool wants = agg || avg;
        if (wants && !pitch_ok(win_pitch, bi.max_n_win)) return -1;
        const size_t pitch = wants ? win_pitch : std::max<size_t>(bi.max_n_win, 1);   // the call's own rows when nothing is handed out
        if (bk.dev.W == 0)
            return empty_bank_answer(c, sg, fmt, S, n_samples, pcm_stride, det, n_det, max_det,
                                     {{agg, S * win_pitch * sizeof(float)}, {avg, S * win_pitch * sizeof(float)}});
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, bk.dev.K, std::max(bk.dev.min_len, 1), det, n_det, max_det, &f)) return -1;
        const size_t out_bytes = S * pitch * sizeof(float);
        float *dg = out_rows(sg, agg, out_bytes, c->ws_agg);
        float *da = dg ? out_rows(sg, avg, out_bytes, c->ws_avg) : nullptr;
        if (!dg || !da) return -1;
        uint32_t *hot = nullptr;
        if (S && pitch) {
            BankScore q;
            q.mfcc = f.dm; q.S = S; q.n_frames = nf; q.win_pitch = pitch; q.stream_wakeword = bi.dev; q.band = (int)config->band_size;
            q.score_mode = (int)config->score_mode; q.score_ref = config->score_ref; q.avg_mode = 2;
            q.gate = (!wants && !(c->flags & RP_CTX_FULL_SCORES)) ? 1 : 0;   // detect-only
            q.threshold = config->threshold; q.avg_threshold = config->avg_threshold;
            q.agg = dg; q.avg = da;
            q.hot = hot = c->hot_flags(S);   // zero: the scan below puts every flag it reads back
            if (!hot || !score_bank(c, bk, q)) return -1;
        }
        const ScanConfig sc = scan_config(*config, 0, true);   // window length, thresholds and the avg test come from the bank, per stream
        if (!detect_scan(c, *config, f.dm, S, nf, bk.dev.K, "scan_bank_kernel", [&](const float *dv, float vm) {
                return launch_scan_bank(c->stream, bk.dev, bi.dev, dg, da, pitch, dv, vm, S, nf, sc, f.dd, f.dn, max_det, hot);
            })) return -1;
        return sg.back_detections(S, max_det, det, f.dd, n_det, f.dn) && sg.back(agg, dg, out_bytes) && sg.back(avg, da, out_bytes) && sg.finish() ? 0 : -1;
    });
}

int rp_batch_detect_bank_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                              const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int set_size, const rp_detector_config *config,
                              rp_batch_detection *det, int32_t *det_wakeword, int32_t *n_det, int max_det, float *agg, float *avg, size_t win_pitch) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!set_size_ok(set_size)) return -1;
        if (!config || (S && (!pcm || !stream_wakewords || !det || !n_det))) { set_last_error("null argument"); return -1; }
        const Bank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_band_ok(bk, (int)config->band_size)) return -1;
        Staged sg(c);
        const size_t nf = rp_mfcc_num_frames(n_samples);
        BankIndices bi;
        if (!stage_bank_indices(c, sg, bk, stream_wakewords, S, set_size, nf, &bi)) return -1;
        const bool wants = agg || avg;
        if (wants && !pitch_ok(win_pitch, bi.max_n_win)) return -1;
        const size_t pitch = wants ? win_pitch : std::max<size_t>(bi.max_n_win, 1);   // the call's own rows when nothing is handed out
        const size_t col = S * (size_t)(max_det > 0 ? max_det : 0) * sizeof(int32_t), slot_bytes = S * (size_t)set_size * pitch * sizeof(float);
        if (bk.dev.W == 0)
            return empty_bank_answer(c, sg, fmt, S, n_samples, pcm_stride, det, n_det, max_det, {{det_wakeword, col}, {agg, slot_bytes}, {avg, slot_bytes}});
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, bk.dev.K, std::max(bk.dev.min_len, 1), det, n_det, max_det, &f)) return -1;
        int32_t *dw = det_wakeword ? static_cast<int32_t *>(sg.out(det_wakeword, col, c->stage_out3)) : nullptr;
        if (det_wakeword && !dw) return -1;
        // the proposals' three rows are the call's own; the per-slot rows exist only when asked for
        const size_t row_bytes = S * pitch * sizeof(float);
        if (!c->ws_agg.reserve(row_bytes + 16) || !c->ws_avg.reserve(row_bytes + 16) || !c->ws_set_ww.reserve(row_bytes + 16)) return -1;
        float *best = c->ws_agg.as<float>(), *best_avg = c->ws_avg.as<float>(), *dg = nullptr, *da = nullptr;
        int32_t *best_ww = c->ws_set_ww.as<int32_t>();
        // (the averaged-template scores travel with the aggregates: a caller that asks for avg alone gets the kernel's aggregate rows too)
        if (wants && !(dg = out_rows(sg, agg, slot_bytes, c->ws_set_agg))) return -1;
        if (avg && !(da = out_rows(sg, avg, slot_bytes, c->ws_set_avg))) return -1;
        uint32_t *hot = nullptr;
        if (S && pitch) {
            BankSetScore q;
            q.mfcc = f.dm; q.S = S; q.n_frames = nf; q.win_pitch = pitch; q.stream_wakewords = bi.dev; q.set_size = set_size; q.band = (int)config->band_size;
            q.score_mode = (int)config->score_mode; q.score_ref = config->score_ref; q.avg_mode = 2;
            q.gate = (!wants && !(c->flags & RP_CTX_FULL_SCORES)) ? 1 : 0;   // detect-only
            q.threshold = config->threshold; q.avg_threshold = config->avg_threshold;
            q.best = best; q.best_avg = best_avg; q.best_ww = best_ww; q.slot_agg = dg; q.slot_avg = da;
            q.hot = hot = c->hot_flags(S);   // zero: the scan below puts every flag it reads back
            if (!hot || !score_bank_sets(c, bk, q)) return -1;
        }
        const ScanConfig sc = scan_config(*config, 0, true);   // window length, thresholds and the avg test come from the bank, per stream
        if (!detect_scan(c, *config, f.dm, S, nf, bk.dev.K, "scan_set_kernel", [&](const float *dv, float vm) {
                return launch_scan_set(c->stream, bk.dev, bi.dev, set_size, best, best_avg, best_ww, pitch, dv, vm, S, nf, sc, f.dd, dw, f.dn, max_det, hot);
            })) return -1;
        if (!sg.back_detections(S, max_det, det, f.dd, n_det, f.dn) || (dw && !sg.back(det_wakeword, dw, col))) return -1;
        return sg.back(agg, dg, slot_bytes) && sg.back(avg, da, slot_bytes) && sg.finish() ? 0 : -1;
    });
}

int rp_mlp_forward_windows_bank(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_model, const float *mfcc, size_t S, size_t n_frames,
                                int precision, float *logits, size_t win_pitch) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (S && !stream_model) { set_last_error("null argument"); return -1; }
        const ModelBank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_precision_ok(precision)) return -1;
        Staged sg(c);
        ModelBankCall q;
        if (!stage_model_indices(c, sg, bk, stream_model, S, n_frames, &q) || !pitch_ok(win_pitch, q.idx.max_n_win, true)) return -1;
        const size_t out_bytes = S * win_pitch * (size_t)bk.dev.label_pitch * sizeof(float);
        if (out_bytes == 0) return sg.finish() ? 0 : -1;
        if (!logits || (n_frames && !mfcc)) { set_last_error("null argument"); return -1; }
        const float *dm = static_cast<const float *>(sg.in(mfcc, S * n_frames * 16 * sizeof(float), c->stage_in));
        float *dl = static_cast<float *>(sg.out(logits, out_bytes, c->stage_out));
        if ((n_frames && !dm) || !dl) return -1;
        if (!bank_logits(c, bk, q, dm, S, n_frames, win_pitch, dl)) return -1;
        return sg.back(logits, dl, out_bytes) && sg.finish() ? 0 : -1;
    });
}

int rp_batch_detect_model_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                               const rp_model_bank *bank, const int32_t *stream_model, const rp_detector_config *config, int precision,
                               rp_batch_detection *det, int32_t *det_label, int32_t *n_det, int max_det) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!config || (S && (!pcm || !stream_model || !det || !n_det))) { set_last_error("null argument"); return -1; }
        const ModelBank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_precision_ok(precision)) return -1;
        if (max_det < 0) { set_last_error("max_det must be >= 0"); return -1; }
        Staged sg(c);
        const size_t nf = rp_mfcc_num_frames(n_samples);
        ModelBankCall q;
        if (!stage_model_indices(c, sg, bk, stream_model, S, nf, &q)) return -1;
        const size_t col = S * (size_t)max_det * sizeof(int32_t);
        if (bk.dev.W == 0) return empty_bank_answer(c, sg, fmt, S, n_samples, pcm_stride, det, n_det, max_det, {{det_label, col}});
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, 16, std::max(bk.min_L, 1), det, n_det, max_det, &f)) return -1;
        int32_t *dl = det_label ? static_cast<int32_t *>(sg.out(det_label, col, c->stage_out3)) : nullptr;
        if (det_label && S && max_det && !dl) return -1;
        const size_t pitch = std::max<size_t>(q.idx.max_n_win, 1), rows = S * pitch;
        if (!c->ws_ring.reserve(rows * (size_t)bk.dev.label_pitch * sizeof(float) + 16) || !c->ws_agg.reserve(rows * sizeof(float) + 16) ||
            !c->ws_avg.reserve(rows * sizeof(float) + 16) || !c->ws_rms.reserve(rows * sizeof(int32_t) + 16)) return -1;
        float *dlog = c->ws_ring.as<float>(), *dg = c->ws_agg.as<float>(), *da = c->ws_avg.as<float>();
        int32_t *dlab = c->ws_rms.as<int32_t>();
        uint32_t *hot = nullptr;
        if (S) {
            if (!bank_logits(c, bk, q, f.dm, S, nf, pitch, dlog)) return -1;
            // nn_score_bank_kernel raises a flag per stream with a window that passed: the scan skips the others and puts the flags back
            hot = c->hot_flags(S);
            if (!hot) return -1;
            if (!hip_ok(launch_nn_score_bank(c->stream, bk.dev, q.idx.dev, dlog, S, nf, pitch, config->score_ref * 10.f, config->avg_threshold != 0.f ? 1 : 0,
                                             config->threshold, config->avg_threshold, dg, da, dlab, hot), "nn_score_bank_kernel")) return -1;
        }
        // window length (countdown L / 2) per stream from the bank's scan entries; their thresholds are -1: the gates were applied above
        const ScanConfig sc = scan_config(*config, 0, true);
        if (!detect_scan(c, *config, f.dm, S, nf, 16, "scan_bank_kernel", [&](const float *dv, float vm) {
                return launch_scan_bank(c->stream, bk.scan, q.idx.dev, dg, da, pitch, dv, vm, S, nf, sc, f.dd, f.dn, max_det, hot);
            })) return -1;
        if (dl && !hip_ok(launch_model_bank_labels(c->stream, f.dd, f.dn, dlab, S, pitch, max_det, dl), "model_bank_labels_kernel")) return -1;
        return sg.back_detections(S, max_det, det, f.dd, n_det, f.dn, det_label, dl) && sg.finish() ? 0 : -1;
    });
}

int rp_mlp_forward_windows_bank_sets(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_models, int set_size, const float *mfcc, size_t S,
                                     size_t n_frames, int precision, float *logits, size_t win_pitch) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!model_set_size_ok(set_size)) return -1;
        if (S && !stream_models) { set_last_error("null argument"); return -1; }
        const ModelBank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_precision_ok(precision)) return -1;
        Staged sg(c);
        ModelBankCall q;
        if (!stage_model_set_indices(c, sg, bk, stream_models, S, set_size, n_frames, &q) || !pitch_ok(win_pitch, q.idx.max_n_win, true)) return -1;
        const size_t out_bytes = S * (size_t)set_size * win_pitch * (size_t)bk.dev.label_pitch * sizeof(float);
        if (out_bytes == 0) return sg.finish() ? 0 : -1;
        if (!logits || (n_frames && !mfcc)) { set_last_error("null argument"); return -1; }
        const float *dm = static_cast<const float *>(sg.in(mfcc, S * n_frames * 16 * sizeof(float), c->stage_in));
        float *dl = static_cast<float *>(sg.out(logits, out_bytes, c->stage_out));
        if ((n_frames && !dm) || !dl) return -1;
        if (!bank_set_logits(c, bk, q, set_size, dm, S, n_frames, win_pitch, dl)) return -1;
        return sg.back(logits, dl, out_bytes) && sg.finish() ? 0 : -1;
    });
}

int rp_batch_detect_model_bank_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                    const rp_model_bank *bank, const int32_t *stream_models, int set_size, const rp_detector_config *config,
                                    int precision, rp_batch_detection *det, int32_t *det_model, int32_t *det_label, int32_t *n_det, int max_det) {
    return guarded([&]() -> int {
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!model_set_size_ok(set_size)) return -1;
        if (!config || (S && (!pcm || !stream_models || !det || !n_det))) { set_last_error("null argument"); return -1; }
        const ModelBank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c || !bank_precision_ok(precision)) return -1;
        if (max_det < 0) { set_last_error("max_det must be >= 0"); return -1; }
        Staged sg(c);
        const size_t nf = rp_mfcc_num_frames(n_samples);
        ModelBankCall q;
        if (!stage_model_set_indices(c, sg, bk, stream_models, S, set_size, nf, &q)) return -1;
        const size_t col = S * (size_t)max_det * sizeof(int32_t);
        if (bk.dev.W == 0) return empty_bank_answer(c, sg, fmt, S, n_samples, pcm_stride, det, n_det, max_det, {{det_model, col}, {det_label, col}});
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, 16, std::max(bk.min_L, 1), det, n_det, max_det, &f)) return -1;
        // the two int32 columns: the caller's arrays on the device, else the halves of one staging buffer
        int32_t *dw = det_model, *dl = det_label;
        if (sg.host && col && (det_model || det_label)) {
            if (!c->stage_out3.reserve(2 * col)) return -1;
            if (det_model) dw = c->stage_out3.as<int32_t>();
            if (det_label) dl = c->stage_out3.as<int32_t>() + S * (size_t)max_det;
        }
        const size_t pitch = std::max<size_t>(q.idx.max_n_win, 1), rows = S * pitch;
        if (!c->ws_ring.reserve(rows * (size_t)set_size * (size_t)bk.dev.label_pitch * sizeof(float) + 16) || !c->ws_agg.reserve(rows * sizeof(float) + 16) ||
            !c->ws_avg.reserve(rows * sizeof(float) + 16) || !c->ws_set_ww.reserve(rows * sizeof(int32_t) + 16) ||
            !c->ws_rms.reserve(rows * sizeof(int32_t) + 16)) return -1;
        float *dlog = c->ws_ring.as<float>(), *best = c->ws_agg.as<float>(), *best_avg = c->ws_avg.as<float>();
        int32_t *best_ww = c->ws_set_ww.as<int32_t>(), *best_label = c->ws_rms.as<int32_t>();
        uint32_t *hot = nullptr;
        if (S) {
            if (!bank_set_logits(c, bk, q, set_size, f.dm, S, nf, pitch, dlog)) return -1;
            // nn_score_model_set_kernel raises a flag per stream with a proposal: the scan skips the others and puts the flags back
            hot = c->hot_flags(S);
            if (!hot) return -1;
            if (!hip_ok(launch_nn_score_model_set(c->stream, bk.dev, q.idx.dev, set_size, dlog, S, nf, pitch, config->score_ref * 10.f,
                                                  config->avg_threshold != 0.f ? 1 : 0, config->threshold, config->avg_threshold, best, best_avg, best_ww,
                                                  best_label, hot), "nn_score_model_set_kernel")) return -1;
        }
        // Lmax(s) (countdown Lmax(s) / 2) from the bank's scan entries; the gates were applied above
        const ScanConfig sc = scan_config(*config, 0, true);
        if (!detect_scan(c, *config, f.dm, S, nf, 16, "scan_model_set_kernel", [&](const float *dv, float vm) {
                return launch_scan_model_set(c->stream, bk.scan, q.idx.dev, set_size, best, best_avg, best_ww, best_label, pitch, dv, vm, S, nf, sc, f.dd, dw, dl,
                                             f.dn, max_det, hot);
            })) return -1;
        if (!sg.back_detections(S, max_det, det, f.dd, n_det, f.dn)) return -1;
        return sg.back(det_model, dw, col) && sg.back(det_label, dl, col) && sg.finish() ? 0 : -1;
    });
}

}  // extern "C"

// ---- mixed sets: stream s holds a row of references of a wakeword bank and a row of models of a model bank on ONE detector
namespace {

// What both mixed calls check first: handles, the two set sizes (0: the side is absent), the arrays, the banks' context (whose device
// becomes current) and add_wakeword's mfcc_size rule (src/detector.rs:316-319) -- a model bank is at 16.  With host arrays every index of
// both rows is checked here, before anything is allocated or launched; the error names stream, slot and side.
struct MixedCall {
    Ctx *c = nullptr;
    const Bank *bk = nullptr;
    const ModelBank *mb = nullptr;
    bool refs_on = false, models_on = false;   // the side has rows AND its bank has entries: only then is anything of it staged, scored or read
};
bool mixed_enter(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int ref_set_size, const rp_model_bank *model_bank,
                 const int32_t *stream_models, int model_set_size, size_t S, MixedCall *m) {
    if (!ctx || !bank || !model_bank) { set_last_error("null handle"); return false; }
    if (ref_set_size < 0 || ref_set_size > RP_WAKEWORD_SET_MAX) {
        set_last_error("ref_set_size " + std::to_string(ref_set_size) + " is outside 0 .. " + std::to_string((int)RP_WAKEWORD_SET_MAX) + " (RP_WAKEWORD_SET_MAX)");
        return false;
    }
    if (model_set_size < 0 || model_set_size > RP_MODEL_SET_MAX) {
        set_last_error("model_set_size " + std::to_string(model_set_size) + " is outside 0 .. " + std::to_string((int)RP_MODEL_SET_MAX) + " (RP_MODEL_SET_MAX)");
        return false;
    }
    if (S && ((ref_set_size && !stream_wakewords) || (model_set_size && !stream_models))) { set_last_error("null argument"); return false; }
    m->bk = bank->impl.get(); m->mb = model_bank->impl.get();
    Ctx *c = ctx->impl.get();
    if (m->bk->ctx != c) { set_last_error("the wakeword bank belongs to another context"); return false; }
    if (m->mb->ctx != c) { set_last_error("the model bank belongs to another context"); return false; }
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return false;
    m->c = c;
    // (an empty bank that was never reserved has a placeholder mfcc_size: a detector without references)
    if ((m->bk->dev.W || m->bk->ceiling) && m->bk->dev.K != 16) {
        set_last_error("Usage of wakewords with different mfcc size is not supported, ignoring wakeword");
        return false;
    }
    if (c->flags & RP_CTX_HOST_POINTERS) {
        if (ref_set_size && !bank_indices_ok(m->bk->dev.W, 0, S, ref_set_size, stream_wakewords, "wakeword index")) return false;
        if (model_set_size && !bank_indices_ok(m->mb->dev.W, 0, S, model_set_size, stream_models, "model index")) return false;
    }
    m->refs_on = ref_set_size > 0 && m->bk->dev.W > 0;
    m->models_on = model_set_size > 0 && m->mb->dev.W > 0;
    return true;
}

}  // namespace

extern "C" {

// rp_frontend_batch_bank_sets over both rows: the level and window of on_wakeword_change over every live slot of either kind, prepared by
// stream_targets_kernel in front of the same per-stream gain kernels
int rp_frontend_batch_mixed_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                 const rp_filters_config *filters, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int ref_set_size,
                                 const rp_model_bank *model_bank, const int32_t *stream_models, int model_set_size, float *pcm_out, size_t out_stride,
                                 float *rms, float *gains) {
    return guarded([&]() -> int {
        MixedCall m;
        if (!mixed_enter(ctx, bank, stream_wakewords, ref_set_size, model_bank, stream_models, model_set_size, S, &m)) return -1;
        Ctx *c = m.c;
        const Bank &bk = *m.bk;
        const ModelBank &mb = *m.mb;
        Staged sg(c);
        BankIndices ri, mi;
        if (m.refs_on && !stage_bank_indices(c, sg, bk, stream_wakewords, S, ref_set_size, 0, &ri)) return -1;
        if (m.models_on && !stage_indices(c, sg, mb.dev.W, mb.min_L, [&](size_t w) { return mb.e[w].L; }, "model index", stream_models, S, model_set_size, 0,
                                          &mi, nullptr, &c->ws_mix_idx)) return -1;
        TargetSide sides[2];
        if (m.refs_on) sides[0] = {ri.dev, ref_set_size, bk.dev.ww, bk.rms_level, bk.dev.W};
        if (m.models_on) sides[1] = {mi.dev, model_set_size, mb.scan.ww, mb.rms_level(), mb.dev.W};
        const int longest = std::max(m.refs_on ? bk.dev.max_len : 0, m.models_on ? mb.max_L : 0);   // the capacity of a stream's ring
        return frontend_batch(c, pcm, fmt, S, n_samples, pcm_stride, filters, 0.f, (size_t)std::max(longest / 3, 1), nullptr, nullptr, pcm_out, out_stride,
                              rms, gains, sides);
    });
}

int rp_batch_detect_mixed_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                               const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int ref_set_size, const rp_model_bank *model_bank,
                               const int32_t *stream_models, int model_set_size, const rp_detector_config *config, int precision,
                               rp_batch_detection *det, int32_t *det_wakeword, int32_t *det_label, int32_t *n_det, int max_det) {
    return guarded([&]() -> int {
        MixedCall m;
        if (!mixed_enter(ctx, bank, stream_wakewords, ref_set_size, model_bank, stream_models, model_set_size, S, &m)) return -1;
        if (!config || (S && (!pcm || !det || !n_det))) { set_last_error("null argument"); return -1; }
        Ctx *c = m.c;
        const Bank &bk = *m.bk;
        const ModelBank &mb = *m.mb;
        if (!bank_band_ok(bk, (int)config->band_size) || !bank_precision_ok(precision)) return -1;
        if (max_det < 0) { set_last_error("max_det must be >= 0"); return -1; }
        Staged sg(c);
        const size_t nf = rp_mfcc_num_frames(n_samples);
        const size_t col = S * (size_t)max_det * sizeof(int32_t);
        // no reference and no model anywhere: every stream is a detector without wakewords
        if (!m.refs_on && !m.models_on)
            return empty_bank_answer(c, sg, fmt, S, n_samples, pcm_stride, det, n_det, max_det, {{det_wakeword, col}, {det_label, col}});
        BankIndices ri;
        ModelBankCall q;
        if (m.refs_on && !stage_bank_indices(c, sg, bk, stream_wakewords, S, ref_set_size, nf, &ri)) return -1;
        if (m.models_on && !stage_model_set_indices(c, sg, mb, stream_models, S, model_set_size, nf, &q, &c->ws_mix_idx)) return -1;
        DetectFront f;
        if (!detect_front(c, sg, pcm, fmt, S, n_samples, pcm_stride, 16, 1, det, n_det, max_det, &f)) return -1;
        // the two int32 columns: the caller's arrays on the device, else the halves of one staging buffer
        int32_t *dw = det_wakeword, *dl = det_label;
        if (sg.host && col && (det_wakeword || det_label)) {
            if (!c->stage_out3.reserve(2 * col)) return -1;
            if (det_wakeword) dw = c->stage_out3.as<int32_t>();
            if (det_label) dl = c->stage_out3.as<int32_t>() + S * (size_t)max_det;
        }
        // Both sides write their proposals for their OWN window counts (each at least the stream's: Lmax(s) is the longer window), into
        // separate workspaces with one pitch
        const size_t pitch = std::max<size_t>(std::max(m.refs_on ? ri.max_n_win : 0, m.models_on ? q.idx.max_n_win : 0), 1), rows = S * pitch;
        if (!c->ws_gain_tab.reserve(gain_targets_bytes(S))) return -1;
        if (m.refs_on && (!c->ws_agg.reserve(rows * sizeof(float) + 16) || !c->ws_avg.reserve(rows * sizeof(float) + 16) ||
                          !c->ws_set_ww.reserve(rows * sizeof(int32_t) + 16))) return -1;
        if (m.models_on && (!c->ws_ring.reserve(rows * (size_t)model_set_size * (size_t)mb.dev.label_pitch * sizeof(float) + 16) ||
                            !c->ws_mix_best.reserve(rows * sizeof(float) + 16) || !c->ws_mix_avg.reserve(rows * sizeof(float) + 16) ||
                            !c->ws_mix_ww.reserve(rows * sizeof(int32_t) + 16) || !c->ws_mix_label.reserve(rows * sizeof(int32_t) + 16))) return -1;
        TargetSide sides[2];
        MixedProposals pr, pm;
        if (m.refs_on) {
            sides[0] = {ri.dev, ref_set_size, bk.dev.ww, bk.rms_level, bk.dev.W};
            pr.bank = bk.dev; pr.rows = ri.dev; pr.set_size = ref_set_size;
            pr.best = c->ws_agg.as<float>(); pr.best_avg = c->ws_avg.as<float>(); pr.best_ww = c->ws_set_ww.as<int32_t>();
        }
        if (m.models_on) {
            sides[1] = {q.idx.dev, model_set_size, mb.scan.ww, mb.rms_level(), mb.dev.W};
            pm.bank = mb.scan; pm.rows = q.idx.dev; pm.set_size = model_set_size;
            pm.best = c->ws_mix_best.as<float>(); pm.best_avg = c->ws_mix_avg.as<float>(); pm.best_ww = c->ws_mix_ww.as<int32_t>();
            pm.best_label = c->ws_mix_label.as<int32_t>();
        }
        uint32_t *hot = nullptr;
        PerStreamGain per;   // (its table is what the scan reads Lmax(s) from)
        if (S) {
            if (!hip_ok(launch_stream_targets(c->stream, sides[0], sides[1], S, c->ws_gain_tab.p, &per), "stream_targets_kernel")) return -1;
            // both scoring kernels raise the same flag per stream with a proposal: the scan skips the others and puts the flags back
            hot = c->hot_flags(S);
            if (!hot) return -1;
            if (m.refs_on) {
                BankSetScore qs;
                qs.mfcc = f.dm; qs.S = S; qs.n_frames = nf; qs.win_pitch = pitch; qs.stream_wakewords = ri.dev; qs.set_size = ref_set_size;
                qs.band = (int)config->band_size; qs.score_mode = (int)config->score_mode; qs.score_ref = config->score_ref; qs.avg_mode = 2;
                qs.gate = (c->flags & RP_CTX_FULL_SCORES) ? 0 : 1;   // detect-only
                qs.threshold = config->threshold; qs.avg_threshold = config->avg_threshold;
                qs.best = c->ws_agg.as<float>(); qs.best_avg = c->ws_avg.as<float>(); qs.best_ww = c->ws_set_ww.as<int32_t>();
                qs.hot = hot;
                if (!score_bank_sets(c, bk, qs)) return -1;
            }
            if (m.models_on) {
                float *dlog = c->ws_ring.as<float>();
                if (!bank_set_logits(c, mb, q, model_set_size, f.dm, S, nf, pitch, dlog)) return -1;
                if (!hip_ok(launch_nn_score_model_set(c->stream, mb.dev, q.idx.dev, model_set_size, dlog, S, nf, pitch, config->score_ref * 10.f,
                                                      config->avg_threshold != 0.f ? 1 : 0, config->threshold, config->avg_threshold, c->ws_mix_best.as<float>(),
                                                      c->ws_mix_avg.as<float>(), c->ws_mix_ww.as<int32_t>(), c->ws_mix_label.as<int32_t>(), hot),
                            "nn_score_model_set_kernel")) return -1;
            }
        }
        // Lmax(s) (countdown Lmax(s) / 2) from the table; the gates were applied by the scoring kernels
        const ScanConfig sc = scan_config(*config, 0, true);
        if (!detect_scan(c, *config, f.dm, S, nf, 16, "scan_mixed_set_kernel", [&](const float *dv, float vm) {
                return launch_scan_mixed_set(c->stream, pr, pm, per.ww, pitch, dv, vm, S, nf, sc, f.dd, dw, dl, f.dn, max_det, hot);
            })) return -1;
        if (!sg.back_detections(S, max_det, det, f.dd, n_det, f.dn)) return -1;
        return sg.back(det_wakeword, dw, col) && sg.back(det_label, dl, col) && sg.finish() ? 0 : -1;
    });
}

}  // extern "C"
