// rp_stream_batch.cpp -- live-stream batches (rp_stream_batch_*): S streams fed a few chunks per call, every stream's state on the device.
// A batch holds shared wakewords (references and / or models), or every stream its own: of a wakeword bank, or of a model bank -- one, or a set --
// or of both banks at once (mixed sets: references and models on one detector per stream).
#include <cmath>
#include <cstring>

#include "rp_capi.h"

using namespace rp;

// one wakeword of a live-stream batch: a reference or a model
struct StreamWakeword {
    const Templates *t = nullptr;
    Model *m = nullptr;
    int none_index = -1, precision = 0;
    float threshold = 0.f, avg_threshold = 0.f;   // the wakeword's own values (the config's where it has none)
    DevBuf agg, avg, label;                       // [S][frames per call] of this wakeword (label: models only)
};

struct rp_stream_batch {
    Ctx *c = nullptr;
    std::vector<std::unique_ptr<StreamWakeword>> ww;  // 1..8 wakewords; the one reference of rp_stream_batch_new
    // made by rp_stream_batch_new: `agg` may be asked for, and its scoring keeps the kernel choice of that entry point (score_reference)
    bool single = false;
    // made by rp_stream_batch_new_bank: stream s holds the one wakeword bank[bank_idx[s]] (`ww` is empty); max_len is then the bank's longest
    // window, the history every stream keeps, and bank_agg / bank_avg [S][frames per call] are the streams' own windows' scores
    // The bank may change under the batch (rp_wakeword_bank_put / _enrol): every call reads bank->dev and bank->rms_level afresh, and the bank
    // counts its batches so that no window longer than max_len gets in (Bank::put_check)
    const Bank *bank = nullptr;
    ~rp_stream_batch() { if (bank) --bank->live_batches; if (mbank) --mbank->live_batches; }
    DevBuf bank_idx, bank_agg, bank_avg;
    // made by rp_stream_batch_new_bank_sets (set_size 1..8; 0: not a sets batch): stream s holds the set bank_idx[s][0 .. set_size), -1 an
    // empty slot; bank_agg / bank_avg are then the slot scores [S][set_size][frames per call] and slot_frames the frames of the last call
    int set_size = 0;
    size_t slot_frames = 0;
    // made by rp_stream_batch_new_model_bank: stream s runs the one model mbank[bank_idx[s]] (`ww` is empty, `bank` null).  max_len is the bank's
    // longest window; bank_agg / bank_avg / bank_label [S][frames per call] are the scores and labels of the streams' own windows, `logits`
    // [S][logit_frames][label_pitch] those of the last call (rp_stream_batch_logits).  The bank may change under the batch (rp_model_bank_put /
    // _train): every call reads mbank->dev afresh; max_len and label_pitch are the batch's own, fixed at creation (the bank's reservation or
    // what it held then), and the bank counts its batches so that no longer window and no larger label count gets in (ModelBank::put_check)
    const ModelBank *mbank = nullptr;
    int label_pitch = 0;
    DevBuf bank_label;
    size_t logit_frames = 0;
    // made by rp_stream_batch_new_model_bank_sets (mbank with set_size 1..8): stream s holds the set of models bank_idx[s][0 .. set_size), -1 an
    // empty slot; bank_agg / bank_avg / bank_label and `logits` are then per slot, [S][set_size][frames per call]([label_pitch])
    size_t slots() const { return set_size ? (size_t)set_size : 1; }
    // made by rp_stream_batch_new_mixed_sets (`mixed`; bank AND mbank set): stream s holds the references bank_idx[s][0 .. set_size) of `bank` and
    // the models model_idx[s][0 .. mset_size) of `mbank` on one detector; either size may be 0 (the side is absent).  max_len is the longer of the
    // two banks' windows (reservations included).  bank_agg / bank_avg are the reference slots' scores [S][set_size][frames per call], m_agg /
    // m_avg / bank_label the model slots' [S][mset_size][..], `logits` [S][mset_size][frames][label_pitch].  gain_tab holds the per-stream table
    // of stream_targets_kernel, written at the start of EVERY call: Lmax(s) for the scoring and scan kernels, the level for the gain normaliser.
    bool mixed = false;
    int mset_size = 0;
    DevBuf model_idx, m_agg, m_avg;
    PerStreamGain mixed_per;   // what the last launch_stream_targets filled (mixed_per.ww: the table)
    int K = 0, max_len = 0, Tmax = 1;             // mfcc_size, max_mfcc_frames (longest wakeword), most templates of a reference
    DevBuf det_ww, det_label, logits, mean, xrows, xs2;
    rp_detector_config cfg{};
    size_t S = 0, max_chunks = 0, chunks_seen = 0, hist_frames = 0;
    bool poisoned = false;   // a launch failed after part of the persistent state had advanced
    // MFCC window: rows of `cap` frames; a call appends its frames behind the `fill` valid ones and only when a row
    // is full are the last max_len-1 frames moved to the front of the other buffer
    int cur = 0;
    size_t cap = 0, fill = 0;
    // previous chunk | new chunks (f32), ping-pong so that one kernel both carries the old chunk and decodes the new
    int pcur = 0;
    size_t last_off = 0;     // where the last chunk of the previous call sits in pcm[pcur]'s rows
    DevBuf pcm[2], mfcc[2], state, scores, vad, list;
    // AudioEncoder of the streams (src/audio/encoder.rs): channel count and, for input that is not 16 kHz, the
    // resampler plan with every stream's previous input frame
    int channels = 1;
    size_t in_len = 480;
    size_t out_len = 480;    // encoded (16 kHz) samples per input frame: 480, or 640 for the 11.025 / 22.05 kHz family
    size_t fpf() const { return out_len / 160; }  // MFCC frames a stream gains per input frame (3 or 4)
    size_t pcm_pitch() const { return 480 + max_chunks * out_len; }  // a pcm row: the last 480 encoded samples of the previous call | the new ones
    const Resampler *rs = nullptr;
    DevBuf rs_prev[2], rs_xs, rs_out;
    int rs_cur = 0;
    // RustpotterConfig.filters of the streams (rp_stream_batch_set_filters): both filters' state by stream, and the chunk levels /
    // gains [S][levels_chunks] of the last call
    bool has_filters = false;
    rp_filters_config filt{};
    float rms_level_ref = 0.f, bq[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int gain_window = 1;
    // rp_stream_batch_set_filters_bank: the gain normaliser of stream s takes its reference level and window size from its own wakeword of the
    // bank, read through bank_idx at the start of every call; gain_window is then the capacity of a stream's ring, the bank's largest window
    bool per_stream_gain = false;
    // rp_stream_batch_set_filters_per_stream: the level and window of stream s come from ALL the bank entries it holds (a set of wakewords or of
    // models, one model, one wakeword), folded by stream_targets_kernel at the start of every call into gain_tab, the per-stream table the same
    // gain kernels then read; a bank that changed under the batch is seen from the next call
    bool prep_gain = false;
    DevBuf gain_tab;
    DevBuf filt_state, lv_rms, lv_gain;
    size_t levels_chunks = 0;
    bool filters_on() const { return has_filters && (filt.gain_normalizer.enabled || filt.band_pass.enabled); }
};

// The prologue of the entry points: null handle -> the batch's device -> (refuse_poisoned) the failed state.  nullptr with the error set.
static Ctx *stream_batch_enter(const rp_stream_batch *b, bool refuse_poisoned) {
    if (!b) { set_last_error("null handle"); return nullptr; }
    if (!hip_ok(hipSetDevice(b->c->device), "hipSetDevice")) return nullptr;
    if (refuse_poisoned && b->poisoned) { set_last_error("stream batch is in a failed state (an earlier call failed half way); free it and create a new one"); return nullptr; }
    return b->c;
}

// buffers of a fresh batch, sized for the current input frame length (30 ms frames: 3 MFCC frames each, 40 ms: 4)
static bool stream_batch_alloc(rp_stream_batch *b) {
    Ctx *c = b->c;
    const size_t S = b->S, fpf = b->fpf(), K = (size_t)b->K;
    b->cap = b->hist_frames + fpf * b->max_chunks * 8;  // compaction every 8 full-size calls
    const size_t pitch = b->cap, rows = S * fpf * b->max_chunks;
    const size_t slack = 64 * K * sizeof(float);  // the DTW band reads up to band_size frames past a row
    const size_t pcm_bytes = S * b->pcm_pitch() * sizeof(float);
    for (auto &w : b->ww)
        if (!w->agg.reserve(rows * sizeof(float) + 16) || !w->avg.reserve(rows * sizeof(float) + 16) ||
            (w->m && !w->label.reserve(rows * sizeof(int32_t) + 16)))
            return false;
    if (b->mixed) {   // a row per reference slot and per model slot; the table of every call
        const size_t rr = rows * (size_t)b->set_size, mr = rows * (size_t)b->mset_size;
        if (!b->bank_agg.reserve(rr * sizeof(float) + 16) || !b->bank_avg.reserve(rr * sizeof(float) + 16) || !b->m_agg.reserve(mr * sizeof(float) + 16) ||
            !b->m_avg.reserve(mr * sizeof(float) + 16) || !b->bank_label.reserve(mr * sizeof(int32_t) + 16) || !b->mean.reserve(mr * 16 * sizeof(float) + 16) ||
            !b->logits.reserve(mr * (size_t)b->label_pitch * sizeof(float) + 16) || !b->gain_tab.reserve(gain_targets_bytes(S))) return false;
    }
    if (!b->mixed && b->bank && (!b->bank_agg.reserve(rows * b->slots() * sizeof(float) + 16) || !b->bank_avg.reserve(rows * b->slots() * sizeof(float) + 16))) return false;
    const size_t mrows = rows * b->slots();   // a batch over model sets: a row per slot
    if (!b->mixed && b->mbank && (!b->bank_agg.reserve(mrows * sizeof(float) + 16) || !b->bank_avg.reserve(mrows * sizeof(float) + 16) ||
                     !b->bank_label.reserve(mrows * sizeof(int32_t) + 16) || !b->mean.reserve(mrows * 16 * sizeof(float) + 16) ||
                     !b->logits.reserve(mrows * (size_t)b->label_pitch * sizeof(float) + 16))) return false;
    if (!b->pcm[0].reserve(pcm_bytes) || !b->pcm[1].reserve(pcm_bytes) || !b->mfcc[0].reserve(S * pitch * K * sizeof(float) + slack) ||
        !b->mfcc[1].reserve(S * pitch * K * sizeof(float) + slack) || !b->state.reserve(S * stream_state_bytes()) ||
        !b->scores.reserve(rows * (size_t)b->Tmax * sizeof(float) + 16) || !b->vad.reserve(rows * sizeof(float) + 16) ||
        !b->list.reserve((rows + 1) * sizeof(uint32_t) + 16))
        return false;
    if (!hip_ok(hipMemsetAsync(b->pcm[0].p, 0, b->pcm[0].cap, c->stream), "hipMemsetAsync") ||
        !hip_ok(hipMemsetAsync(b->pcm[1].p, 0, b->pcm[1].cap, c->stream), "hipMemsetAsync") ||
        !hip_ok(hipMemsetAsync(b->mfcc[0].p, 0, b->mfcc[0].cap, c->stream), "hipMemsetAsync") ||
        !hip_ok(hipMemsetAsync(b->mfcc[1].p, 0, b->mfcc[1].cap, c->stream), "hipMemsetAsync") ||
        !hip_ok(launch_stream_state_init(c->stream, b->state.p, S), "stream_state_init_kernel"))
        return false;
    b->cur = 0; b->fill = b->hist_frames;  // an all-zero history nobody scores against (frames < 0)
    b->pcur = 0; b->last_off = 0;
    return true;
}

// Both constructors; single: rp_stream_batch_new, a batch of its one reference
static int stream_batch_new(rp_ctx *ctx, size_t n_wakewords, const rp_wakeword_spec *wakewords, int mfcc_size, const rp_detector_config *config,
                            size_t S, size_t max_chunks_per_call, bool single, rp_stream_batch **out) {
    return guarded([&]() -> int {
        if (!ctx) { set_last_error("null handle"); return -1; }
        if (!config || !out || !wakewords) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        Ctx *c = ctx->impl.get();
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        if (S == 0 || max_chunks_per_call == 0) { set_last_error("rp_stream_batch_new: S and max_chunks_per_call must be >= 1"); return -1; }
        if (n_wakewords < 1 || n_wakewords > (size_t)kScanMaxWakewords) { set_last_error("rp_stream_batch_new_multi: 1..8 wakewords"); return -1; }
        if (mfcc_size < 1) { set_last_error("rp_stream_batch_new_multi: mfcc_size must be >= 1"); return -1; }
        std::unique_ptr<rp_stream_batch> b(new rp_stream_batch());
        b->c = c; b->single = single; b->cfg = *config; b->S = S; b->max_chunks = max_chunks_per_call;
        b->K = mfcc_size; b->max_len = 0; b->Tmax = 1;
        for (size_t j = 0; j < n_wakewords; ++j) {
            const rp_wakeword_spec &w = wakewords[j];
            if ((w.templates != nullptr) == (w.model != nullptr)) { set_last_error("rp_stream_batch_new_multi: every wakeword is a reference OR a model"); return -1; }
            std::unique_ptr<StreamWakeword> e(new StreamWakeword());
            e->threshold = std::isnan(w.threshold) ? config->threshold : w.threshold;
            e->avg_threshold = std::isnan(w.avg_threshold) ? config->avg_threshold : w.avg_threshold;
            if (w.templates) {
                e->t = w.templates->impl.get();
                // (rp_stream_batch_new has never asked where its reference was created)
                if (!single && e->t->ctx != c) { set_last_error("rp_stream_batch_new_multi: the wakewords must have been created on this context"); return -1; }
                // add_wakeword, src/detector.rs:316-319
                if (e->t->dev.K != mfcc_size) { set_last_error("Usage of wakewords with different mfcc size is not supported, ignoring wakeword"); return -1; }
                b->max_len = std::max(b->max_len, e->t->dev.max_len);
                b->Tmax = std::max(b->Tmax, e->t->dev.T);
            } else {
                e->m = w.model->impl.get();
                if (e->m->ctx != c) { set_last_error("rp_stream_batch_new_multi: the wakewords must have been created on this context"); return -1; }
                const int nl = (int)e->m->dims.size() - 1;
                if (e->m->dims[0] % mfcc_size != 0) { set_last_error("Usage of wakewords with different mfcc size is not supported, ignoring wakeword"); return -1; }
                if (w.none_index >= e->m->dims[nl]) { set_last_error("none_index out of range"); return -1; }
                if (!mlp_precision_ok(w.precision)) return -1;
                if (!e->m->mfma_ok && w.precision == RP_MLP_BF16) { set_last_error("this layer-1 shape has no bf16 MFMA kernel"); return -1; }
                e->none_index = w.none_index; e->precision = w.precision;
                b->max_len = std::max(b->max_len, e->m->dims[0] / mfcc_size);
            }
            b->ww.push_back(std::move(e));
        }
        if (!c->tables_for(b->K)) return -1;
        b->hist_frames = (size_t)b->max_len - 1;   // on_wakeword_change, src/detector.rs:328-334: the longest wakeword sets the window
        if (!stream_batch_alloc(b.get())) return -1;
        *out = b.release();
        return 0;
    });
}

// Wakeword indices of streams first .. first + n - 1 of a batch over a bank (set_size 0: one index a stream).  A host array
// (RP_CTX_HOST_POINTERS) is checked (bank_indices_ok); a device array is taken as it is and the kernels treat an index outside [0, W) as -1,
// as the bank calls do.
static bool batch_indices_ok(const Ctx *c, const Bank &bk, size_t first, size_t n, int set_size, const int32_t *idx) {
    return !(c->flags & RP_CTX_HOST_POINTERS) || bank_indices_ok(bk.dev.W, first, n, set_size, idx);
}
// ... -> the batch's own device copy (a sets batch: rows of set_size indices)
// (dst, row: the batch's array and its row length -- bank_idx with slots() but for the model rows of a mixed batch)
static bool indices_put(rp_stream_batch *b, DevBuf &dst, size_t row, size_t first, size_t n, const int32_t *idx) {
    Ctx *c = b->c;
    const bool host = (c->flags & RP_CTX_HOST_POINTERS) != 0;
    if (!dst.reserve(b->S * row * sizeof(int32_t) + 16)) return false;
    if (row == 0 || n == 0) return true;
    if (!hip_ok(hipMemcpyAsync(dst.as<int32_t>() + first * row, idx, n * row * sizeof(int32_t), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream),
                "hipMemcpyAsync(wakeword indices)")) return false;
    // the caller's host array is the caller's again when the call returns
    return !host || hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
}
static bool bank_indices_put(rp_stream_batch *b, size_t first, size_t n, const int32_t *idx) { return indices_put(b, b->bank_idx, b->slots(), first, n, idx); }

// The per-stream table (Lmax(s), level, idx) of this call, folded over the rows of whichever banks the batch has -- one short launch, so a
// bank that changed under the batch is seen from this call on.  A batch over mixed sets: both rows (a side without rows, or whose bank is
// empty, is absent), at the start of every call -- the scoring and scan kernels read Lmax(s) from it; refuses banks that outgrew what the
// batch was sized for.  The other kinds: their one bank, and only for the gain normaliser.
static bool stream_targets(rp_stream_batch *b, PerStreamGain *per) {
    TargetSide first, second;
    if (b->mixed) {
        const Bank &bk = *b->bank;
        const ModelBank &mb = *b->mbank;
        if ((bk.dev.W && (bk.dev.K != 16 || bk.dev.max_len > b->max_len)) || (mb.dev.W && (mb.max_L > b->max_len || mb.dev.label_pitch != b->label_pitch))) {
            set_last_error("stream batch: a bank outgrew what the batch was sized for");
            return false;
        }
        if (b->set_size && bk.dev.W) first = {b->bank_idx.as<int32_t>(), b->set_size, bk.dev.ww, bk.rms_level, bk.dev.W};
        if (b->mset_size && mb.dev.W) second = {b->model_idx.as<int32_t>(), b->mset_size, mb.scan.ww, mb.rms_level(), mb.dev.W};
    } else if (b->mbank) first = {b->bank_idx.as<int32_t>(), (int)b->slots(), b->mbank->scan.ww, b->mbank->rms_level(), b->mbank->dev.W};
    else first = {b->bank_idx.as<int32_t>(), (int)b->slots(), b->bank->dev.ww, b->bank->rms_level, b->bank->dev.W};
    return hip_ok(launch_stream_targets(b->c->stream, first, second, b->S, b->gain_tab.p, per), "stream_targets_kernel");
}

// what the MFCC front of a call reads: the caller's chunks where they lie on the device, or the resampler's 16 kHz output
struct StreamPcm { const void *p; int fmt, channels; size_t stride; };

// Encode stage (AudioEncoder): previous input frame | new input frames -> 16 kHz when the input is not (the resampler never resets,
// src/detector.rs:290-302).  Owns rs_cur.
static bool stream_encode(rp_stream_batch *b, size_t n_chunks, StreamPcm *in) {
    if (!b->rs) return true;
    const size_t new_len = n_chunks * b->out_len;
    float *ro = b->rs_out.as<float>();
    if (!resample_rows(b->c, b->rs->dev, in->p, in->fmt, in->channels, in->stride, b->rs_prev[b->rs_cur].as<float>(),
                       b->rs_prev[b->rs_cur ^ 1].as<float>(), b->S, n_chunks, b->rs_xs, b->max_chunks, ro, new_len)) return false;
    b->rs_cur ^= 1;
    *in = StreamPcm{ro, 3, 1, new_len};
    return true;
}

// what the frames stage hands on: the MFCC rows (b->cap frames a stream) with `fill` valid frames in front of this call's new ones, and the
// [history chunk | new chunks] f32 rows when the input was staged (nullptr: it was read where it lies)
struct NewFrames {
    float *rows = nullptr; size_t fill = 0; const float *staged = nullptr;
    size_t first_win(const rp_stream_batch *b) const { return fill - b->hist_frames; }  // the window that ends at the first new frame
};

// Frames stage: the call's chunks to MFCC frames behind the valid ones.  Owns pcur / last_off (the history chunk) and cur / fill (the rows).
static bool stream_frames(rp_stream_batch *b, const MfccTablesDev &tb, const StreamPcm &in, size_t n_chunks, NewFrames *f) {
    Ctx *c = b->c;
    const size_t S = b->S, K = (size_t)b->K, new_len = n_chunks * b->out_len, n_new = b->fpf() * n_chunks, hist = b->hist_frames;
    const size_t pitch = b->cap, pcm_pitch = b->pcm_pitch();
    const float *hp_old = b->pcm[b->pcur].as<float>();
    float *hp = b->pcm[b->pcur ^ 1].as<float>();
    auto stage = [&] {   // previous chunk | new chunks (first channel), decoded to f32
        return hip_ok(launch_stream_stage(c->stream, in.p, in.fmt, in.channels, S, new_len, in.stride, hp_old, b->last_off, hp, pcm_pitch), "stream_stage_kernel");
    };
    // 16 kHz mono input is read where it lies: the MFCC kernel takes [history chunk | new chunks] from two buffers and
    // leaves the last chunk as the next call's history.  Other inputs are staged into one row per stream first.
    bool staged = b->filters_on() || b->rs || in.channels != 1;
    if (b->mixed && !stream_targets(b, &b->mixed_per)) return false;   // every call, filters or not
    if (b->filters_on()) {
        // with filters, ONE launch in the place of launch_stream_stage: history chunk | the new chunks decoded and filtered, levels kept
        const rp_gain_normalization_config &g = b->filt.gain_normalizer;
        PerStreamGain per;
        if (b->mixed) per = b->mixed_per;
        else if (b->prep_gain) { if (!stream_targets(b, &per)) return false; }
        else if (b->per_stream_gain) { per.stream_wakeword = b->bank_idx.as<int32_t>(); per.ww = b->bank->dev.ww; per.rms_level = b->bank->rms_level; per.W = b->bank->dev.W; }
        per.has_fixed_ref = g.has_gain_ref ? 1 : 0; per.fixed_ref = g.gain_ref;   // fixed_rms_level, gain_normalizer_filter.rs:56-66
        if (!hip_ok(launch_stream_filters(c->stream, in.p, in.fmt, in.channels, S, n_chunks, in.stride, hp_old, b->last_off, hp, pcm_pitch,
                                          g.enabled ? 1 : 0, b->rms_level_ref, g.min_gain, g.max_gain, b->gain_window,
                                          b->filt.band_pass.enabled ? 1 : 0, b->bq[0], b->bq[1], b->bq[2], b->bq[3], b->bq[4],
                                          b->filt_state.as<float>(), b->lv_rms.as<float>(), b->lv_gain.as<float>(),
                                          b->per_stream_gain ? &per : nullptr), "stream_filters_kernel")) return false;
    } else if (staged && !stage()) return false;
    // MFCC window rows: [.. valid frames .. | the 3*n_chunks new frames]; a full row keeps its last max_len-1 frames
    if (b->fill + n_new > b->cap) {
        if (!hip_ok(launch_carry_rows(c->stream, b->mfcc[b->cur].as<float>(), S, pitch * K, (b->fill - hist) * K, hist * K,
                                      b->mfcc[b->cur ^ 1].as<float>(), pitch * K), "carry_rows_kernel")) return false;
        b->cur ^= 1; b->fill = hist;
    }
    float *now = b->mfcc[b->cur].as<float>();
    const size_t fill = b->fill;
    if (!staged) {
        c->time_begin(kKernelMfcc);
        hipError_t e = launch_mfcc_stream(c->stream, tb, in.p, in.fmt, S, n_chunks, in.stride, hp_old + b->last_off, pcm_pitch, hp, pitch, now + fill * K);
        c->time_end();
        if (e == hipErrorNotSupported) {  // rows that do not allow 4-sample loads
            if (!stage()) return false;
            staged = true;
        } else {
            if (!hip_ok(e, "mfcc_kernel")) return false;
            b->pcur ^= 1; b->last_off = 0;  // hist_out: the last chunk of this call at the start of the other buffer's rows
        }
    }
    if (staged) {
        b->pcur ^= 1; b->last_off = new_len;  // the last 480 samples of this call are the extractor history of the next
        if (!timed(c, kKernelMfcc, "mfcc_kernel", [&] { return launch_mfcc(c->stream, tb, hp, S, 480 + new_len, pcm_pitch, 0, n_new, pitch, now + fill * K); }))
            return false;
    }
    b->fill += n_new;
    f->rows = now; f->fill = fill; f->staged = staged ? hp : nullptr;
    return true;
}

// Levels stage: filters configured but both off -- the launches of an unfiltered call, and the levels of its chunks for
// rp_stream_batch_levels (with a filter on, stream_filters_kernel has written them).  Owns levels_chunks.
static bool stream_levels(rp_stream_batch *b, const StreamPcm &in, const NewFrames &f, size_t n_chunks) {
    if (!b->has_filters) return true;
    hipStream_t st = b->c->stream;
    if (!b->filters_on() && !hip_ok(f.staged ? launch_chunk_rms(st, f.staged + 480, 3, b->S, n_chunks, b->pcm_pitch(), b->lv_rms.as<float>())
                                             : launch_chunk_rms(st, in.p, in.fmt, b->S, n_chunks, in.stride, b->lv_rms.as<float>()),
                                    "chunk_rms_kernel")) return false;
    b->levels_chunks = n_chunks;
    return true;
}

// One reference wakeword's scores of this call's n_new windows per stream -> w.agg / w.avg, entered as wakeword j of the scan.  The window
// starts where the longest wakeword's does and this one scores its oldest frames (wakeword_comp.rs:22-27).
static bool score_reference(rp_stream_batch *b, StreamWakeword &w, const NewFrames &f, size_t n_new, bool detect_only, ScanWakewords &sw, size_t j) {
    const TemplatesDev &td = w.t->dev;
    const bool do_avg = td.has_avg && w.avg_threshold != 0.f;  // wakeword_comp.rs:85
    DtwScore q;
    q.t = &td; q.mfcc = f.rows; q.S = b->S; q.frame_pitch = b->cap; q.first_win = f.first_win(b); q.n_win = n_new; q.band = b->cfg.band_size;
    q.score_ref = b->cfg.score_ref; q.with_avg = do_avg; q.detect_only = detect_only;
    q.avg_threshold = w.avg_threshold; q.threshold = w.threshold; q.score_mode = (int)b->cfg.score_mode;
    q.scores = b->scores.as<float>(); q.avg = do_avg ? w.avg.as<float>() : nullptr; q.agg = w.agg.as<float>(); q.gate_list = b->list.as<uint32_t>();
    if (b->single) {
        // (a single live stream with a handful of windows skips the gate's three passes: the batch kernels score it when the matrix-core
        // kernel serves its templates (a stream's bits must not depend on the batch it is in), else one wave per DTW)
        q.gate_one_stream = false; q.fuse_max = true;
    }
    sw.agg[j] = q.agg; sw.avg[j] = q.avg; sw.threshold[j] = w.threshold; sw.avg_threshold[j] = w.avg_threshold; sw.label[j] = nullptr;
    return dtw_score(*b->c, q);
}

// The same for a wakeword model: logits of the windows, then nn_score_kernel's scores and labels
static bool score_model(rp_stream_batch *b, StreamWakeword &w, const NewFrames &f, size_t n_new, ScanWakewords &sw, size_t j) {
    Ctx *c = b->c;
    Model &m = *w.m;
    const int K = b->K, L = m.dims[0] / K, n_labels = m.dims.back();
    const size_t rows = b->S * n_new;
    if (!b->logits.reserve(rows * (size_t)n_labels * sizeof(float) + 16)) return false;
    float *dlog = b->logits.as<float>();
    // window i of stream s starts at frame s * pitch + i from the first frame the longest wakeword scores
    if (!window_logits(c, m, f.rows + f.first_win(b) * K, b->S, b->cap, n_new, L, K, w.precision, dlog, b->mean, b->xrows, b->xs2, true))
        return false;
    float *dg = w.agg.as<float>(), *da = w.avg.as<float>();
    int32_t *dlab = w.label.as<int32_t>();
    sw.agg[j] = dg; sw.avg[j] = da; sw.label[j] = dlab;
    sw.threshold[j] = -1.f; sw.avg_threshold[j] = -1.f;  // the gates were applied by nn_score_kernel (>=, not >)
    return hip_ok(launch_nn_score(c->stream, dlog, rows, n_labels, w.none_index, b->cfg.score_ref * 10.f, w.avg_threshold != 0.f ? 1 : 0,
                                  w.threshold, w.avg_threshold, dg, da, dlab), "nn_score_kernel");
}

// The live tail: VAD values of this call's n_new frames per stream (from `frames`, rows b->cap frames apart) when vad_mode is on, then
// the timed scan that carries every stream's state machine on over the wakewords `sw` (dw / dl: each detection's wakeword and label)
// (a batch over a bank: every stream's own wakeword, scores in bank_agg / bank_avg; `sw` is not read)
static bool live_scan(rp_stream_batch *b, const float *frames, size_t n_new, const ScanWakewords &sw, BatchDetection *dd, int32_t *dw,
                      int32_t *dl, int32_t *dn, int max_det) {
    Ctx *c = b->c;
    float *dv = nullptr;
    if (b->cfg.vad_mode != RP_VAD_NONE) {
        dv = b->vad.as<float>();
        if (!hip_ok(launch_vad_value_rows(c->stream, frames, b->S, n_new, b->cap, b->K, dv), "vad_value_kernel")) return false;
    }
    const float vm = vad_mode_value(b->cfg.vad_mode);
    const long long f0 = (long long)b->fpf() * (long long)b->chunks_seen - 3;
    if (b->mixed) {   // Lmax(s) from this call's table; the references' own thresholds from the bank, the models' gates applied by nn_score_set_stream_kernel
        const ScanConfig sc = scan_config(b->cfg, 0, true, (int)b->fpf());
        return timed(c, kKernelScan, "scan_mixed_set_stream_kernel", [&] {
            return launch_scan_mixed_set_stream(c->stream, b->bank->dev, b->bank_idx.as<int32_t>(), b->set_size, b->mbank->scan, b->model_idx.as<int32_t>(),
                                                b->mset_size, b->mixed_per.ww, b->bank_agg.as<float>(), b->bank_avg.as<float>(), b->m_agg.as<float>(),
                                                b->m_avg.as<float>(), b->bank_label.as<int32_t>(), dv, vm, b->S, f0, (int)n_new, sc, b->state.p, dd, dw, dl, dn,
                                                max_det);
        });
    }
    if (b->mbank) {
        // window length (countdown L / 2) per stream from the bank's scan entries; their thresholds are -1: nn_score_bank_stream_kernel applied the gates
        const ScanConfig sc = scan_config(b->cfg, 0, true, (int)b->fpf());
        if (b->set_size)   // Lmax(s) from the scan entries of the stream's set; per frame the best proposal of its slots
            return timed(c, kKernelScan, "scan_model_set_stream_kernel", [&] {
                return launch_scan_model_set_stream(c->stream, b->mbank->scan, b->bank_idx.as<int32_t>(), b->set_size, b->bank_agg.as<float>(),
                                                    b->bank_avg.as<float>(), b->bank_label.as<int32_t>(), dv, vm, b->S, f0, (int)n_new, sc, b->state.p, dd, dw, dl,
                                                    dn, max_det);
            });
        return timed(c, kKernelScan, "scan_bank_stream_kernel", [&] {
            return launch_scan_bank_stream(c->stream, b->mbank->scan, b->bank_idx.as<int32_t>(), b->bank_agg.as<float>(), b->bank_avg.as<float>(), dv, vm,
                                           b->S, f0, (int)n_new, sc, b->state.p, dd, dw, dl, dn, max_det, b->bank_label.as<int32_t>());
        });
    }
    if (b->bank) {
        const ScanConfig sc = scan_config(b->cfg, 0, true, (int)b->fpf());   // window length, thresholds and the avg test come from the bank, per stream
        if (b->set_size)
            return timed(c, kKernelScan, "scan_set_stream_kernel", [&] {
                return launch_scan_set_stream(c->stream, b->bank->dev, b->bank_idx.as<int32_t>(), b->set_size, b->bank_agg.as<float>(), b->bank_avg.as<float>(),
                                              dv, vm, b->S, f0, (int)n_new, sc, b->state.p, dd, dw, dl, dn, max_det);
            });
        return timed(c, kKernelScan, "scan_bank_stream_kernel", [&] {
            return launch_scan_bank_stream(c->stream, b->bank->dev, b->bank_idx.as<int32_t>(), b->bank_agg.as<float>(), b->bank_avg.as<float>(), dv, vm,
                                           b->S, f0, (int)n_new, sc, b->state.p, dd, dw, dl, dn, max_det);
        });
    }
    const ScanConfig sc = scan_config(b->cfg, b->max_len, false, (int)b->fpf());
    return timed(c, kKernelScan, "scan_stream_kernel", [&] {
        return launch_scan_stream_multi(c->stream, sw, dv, vm, b->S, f0, (int)n_new, sc, b->state.p, dd, dw, dl, dn, max_det);
    });
}

// A batch over a wakeword bank, or the reference side of a batch over mixed sets: every stream's n_new new windows against its own wakeword,
// or every slot of its set, -> bank_agg / bank_avg.  table: the per-stream table of a mixed batch, whose windows are Lmax(s) frames with the
// COMBINED Lmax(s); null: the bank's own.  band_size 0: no cell lies in the band and every score is 0 (dtw.rs:64-75); an empty bank: no
// stream has a wakeword -- zero rows either way, as rp_batch_detect_bank.
static bool score_bank_stream(rp_stream_batch *b, const NewFrames &f, size_t n_new, bool detect_only, const BankWakeword *table) {
    Ctx *c = b->c;
    const BankDev &bd = b->bank->dev;
    const size_t bytes = b->S * b->slots() * n_new * sizeof(float);
    b->slot_frames = n_new;
    if (b->cfg.band_size == 0 || bd.W == 0)
        return hip_ok(hipMemsetAsync(b->bank_agg.p, 0, bytes, c->stream), "hipMemsetAsync") && hip_ok(hipMemsetAsync(b->bank_avg.p, 0, bytes, c->stream), "hipMemsetAsync");
    BankStreamScore q;
    q.mfcc = f.rows; q.S = b->S; q.frame_pitch = b->cap; q.first_new = f.fill; q.n_new = n_new; q.stream_wakeword = b->bank_idx.as<int32_t>();
    q.band = (int)b->cfg.band_size; q.score_mode = (int)b->cfg.score_mode; q.score_ref = b->cfg.score_ref; q.gate = detect_only ? 1 : 0;
    q.avg_threshold = b->cfg.avg_threshold; q.agg = b->bank_agg.as<float>(); q.avg = b->bank_avg.as<float>();
    const DtwWork wk = c->dtw_work();
    q.fix = wk.fix;
    if (table) {
        dtw_mark(wk, kDtwRanMixedSetsStream);
        return timed(c, kKernelDtw, "dtw_mixed_stream_kernel", [&] { return launch_dtw_set_stream(c->stream, bd, q, b->set_size, table, b->max_len); });
    }
    if (b->set_size) {   // every slot of every stream's set is a row
        dtw_mark(wk, kDtwRanBankSetsStream);
        return timed(c, kKernelDtw, "dtw_set_stream_kernel", [&] { return launch_dtw_set_stream(c->stream, bd, q, b->set_size); });
    }
    dtw_mark(wk, kDtwRanBankStream);
    return timed(c, kKernelDtw, "dtw_bank_stream_kernel", [&] { return launch_dtw_bank_stream(c->stream, bd, q); });
}

// A batch over a model bank, or the model side of a batch over mixed sets: the logits of every stream's n_new new windows with its own model,
// or every slot of its set (one forward launch, inside the context's kKernelMlp bracket), then their scores and labels -> agg / avg /
// bank_label.  idx, set_size (0: one model per stream): the side's rows; table as for score_bank_stream.  An empty bank: no stream has a
// model, nothing runs and the scan reports nothing.
static bool score_model_bank_stream(rp_stream_batch *b, const NewFrames &f, size_t n_new, const int32_t *idx, int set_size, float *agg, float *avg,
                                    const BankWakeword *table) {
    Ctx *c = b->c;
    const ModelBank &bk = *b->mbank;
    b->logit_frames = n_new;
    // no model yet (a reserved empty bank): rp_stream_batch_logits answers zero rows
    if (bk.dev.W == 0)
        return !b->label_pitch || hip_ok(hipMemsetAsync(b->logits.p, 0, b->S * (size_t)std::max(set_size, 1) * n_new * (size_t)b->label_pitch * sizeof(float), c->stream), "hipMemsetAsync");
    if (bk.dev.label_pitch != b->label_pitch || bk.max_L > b->max_len) { set_last_error("stream batch: the model bank outgrew what the batch was sized for"); return false; }
    float *mean = b->mean.as<float>(), *dlog = b->logits.as<float>();
    const float ref10 = b->cfg.score_ref * 10.f;
    const int calc_avg = b->cfg.avg_threshold != 0.f ? 1 : 0;
    if (set_size) {   // every slot of every stream's set is a row; Lmax(s) is read from the bank, or from the table, in this call
        if (table) {
            if (!hip_ok(launch_window_means_mixed_stream(c->stream, bk.dev, bk.max_L, b->max_len, idx, set_size, table, f.rows, b->S, b->cap, f.fill, n_new, mean),
                        "window_means_mixed_stream_kernel")) return false;
            if (!timed(c, kKernelMlp, "mlp_mixed_stream_kernel", [&] {
                    return launch_mlp_mixed_stream(c->stream, bk.dev, bk.max_L, b->max_len, idx, set_size, table, f.rows, b->S, b->cap, f.fill, n_new, mean, dlog); }))
                return false;
        } else {
            if (!hip_ok(launch_window_means_set_stream(c->stream, bk.dev, bk.max_L, idx, set_size, f.rows, b->S, b->cap, f.fill, n_new, mean),
                        "window_means_set_stream_kernel")) return false;
            if (!timed(c, kKernelMlp, "mlp_set_stream_kernel", [&] {
                    return launch_mlp_set_stream(c->stream, bk.dev, bk.max_L, idx, set_size, f.rows, b->S, b->cap, f.fill, n_new, mean, dlog); })) return false;
        }
        return hip_ok(launch_nn_score_set_stream(c->stream, bk.dev, idx, set_size, dlog, b->S, n_new, ref10, calc_avg, b->cfg.threshold, b->cfg.avg_threshold,
                                                 agg, avg, b->bank_label.as<int32_t>()), "nn_score_set_stream_kernel");
    }
    if (!hip_ok(launch_window_means_bank_stream(c->stream, bk.dev, bk.max_L, idx, f.rows, b->S, b->cap, f.fill, n_new, mean), "window_means_bank_stream_kernel"))
        return false;
    if (!timed(c, kKernelMlp, "mlp_bank_stream_kernel", [&] {
            return launch_mlp_bank_stream(c->stream, bk.dev, bk.max_L, idx, f.rows, b->S, b->cap, f.fill, n_new, mean, dlog); })) return false;
    return hip_ok(launch_nn_score_bank_stream(c->stream, bk.dev, idx, dlog, b->S, n_new, ref10, calc_avg, b->cfg.threshold, b->cfg.avg_threshold, agg, avg,
                                              b->bank_label.as<int32_t>()), "nn_score_bank_stream_kernel");
}

// Score + scan stage: scores of this call's n_new windows per stream for every wakeword, then the state machine over all of them.
// detect_only: nobody reads the per-window arrays.
static bool stream_score_and_scan(rp_stream_batch *b, Staged &sg, const NewFrames &f, size_t n_new, bool detect_only, BatchDetection *dd,
                                  int32_t *dn, int max_det, int32_t *det_wakeword, int32_t *det_label) {
    ScanWakewords sw{};
    sw.n = (int)b->ww.size();
    if (b->mixed) {   // each side that has rows; every window Lmax(s) frames long with the combined Lmax(s) of this call's table
        const BankWakeword *table = b->mixed_per.ww;
        b->slot_frames = b->logit_frames = n_new;
        if (b->set_size && !score_bank_stream(b, f, n_new, detect_only, table)) return false;
        if (b->mset_size && !score_model_bank_stream(b, f, n_new, b->model_idx.as<int32_t>(), b->mset_size, b->m_agg.as<float>(), b->m_avg.as<float>(), table))
            return false;
    } else if (b->bank && !score_bank_stream(b, f, n_new, detect_only, nullptr)) return false;
    else if (b->mbank && !score_model_bank_stream(b, f, n_new, b->bank_idx.as<int32_t>(), b->set_size, b->bank_agg.as<float>(), b->bank_avg.as<float>(), nullptr))
        return false;
    for (size_t j = 0; j < b->ww.size(); ++j)
        if (!(b->ww[j]->t ? score_reference(b, *b->ww[j], f, n_new, detect_only, sw, j) : score_model(b, *b->ww[j], f, n_new, sw, j))) return false;
    const size_t col = b->S * (size_t)max_det * sizeof(int32_t);
    int32_t *dw = det_wakeword ? static_cast<int32_t *>(sg.out(det_wakeword, col, b->det_ww)) : nullptr;
    int32_t *dl = det_label ? static_cast<int32_t *>(sg.out(det_label, col, b->det_label)) : nullptr;
    if ((det_wakeword && !dw) || (det_label && !dl)) return false;
    return live_scan(b, f.rows + f.fill * b->K, n_new, sw, dd, dw, dl, dn, max_det) && (!dw || sg.back(det_wakeword, dw, col)) &&
           (!dl || sg.back(det_label, dl, col));
}

// Both live entry points.  A call advances device-resident state launch by launch (resampler tail, history chunk, MFCC rows, scan
// state); a failure after the first such step cannot be rolled back, so the batch refuses further work instead of pairing the wrong
// history with later chunks.
static int stream_batch_process(rp_stream_batch *b, const void *pcm, rp_sample_format fmt, size_t n_chunks, size_t pcm_stride,
                                rp_batch_detection *det, int32_t *n_det, int max_det, float *agg, int32_t *det_wakeword, int32_t *det_label) {
    bool touched = false;
    const int r = guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (n_chunks == 0 || n_chunks > b->max_chunks) { set_last_error("rp_stream_batch_process: n_chunks out of range"); return -1; }
        const size_t in_chunk = b->in_len * (size_t)b->channels;
        if (pcm_stride < n_chunks * in_chunk) { set_last_error("pcm_stride smaller than n_chunks * samples per chunk"); return -1; }
        if (!sample_format_ok(fmt)) return -1;
        if (b->mixed && agg) {
            set_last_error("rp_stream_batch_process: a batch over mixed sets has no single aggregate per window; rp_stream_batch_slot_scores returns the reference "
                           "slots' scores, rp_stream_batch_logits the model slots' logits");
            return -1;
        }
        if (b->mbank && agg) {
            set_last_error("rp_stream_batch_process: a batch over a model bank has no aggregate per window; its per-window output is the logits (rp_stream_batch_logits)");
            return -1;
        }
        if (!b->single && (!b->bank || b->set_size) && agg) { set_last_error("rp_stream_batch_process: a batch of several wakewords has no single aggregate per window"); return -1; }
        const MfccTablesDev *tb = c->tables_for(b->K);
        if (!tb) return -1;
        const size_t S = b->S, n_new = b->fpf() * n_chunks;
        Staged sg(c);
        const void *dp = sg.in(pcm, S * pcm_stride * sample_bytes(fmt), c->stage_in);
        BatchDetection *dd = static_cast<BatchDetection *>(sg.out(det, S * (size_t)max_det * sizeof(BatchDetection), c->stage_out));
        int32_t *dn = static_cast<int32_t *>(sg.out(n_det, S * sizeof(int32_t), c->stage_out2));
        if (!dp || !dd || !dn) { if (!pcm || !det || !n_det) set_last_error("null argument"); return -1; }
        touched = true;  // from here on every launch moves persistent state
        StreamPcm in{dp, (int)fmt, b->channels, pcm_stride};
        NewFrames f;
        // unless the caller wants every window's aggregate, the gate may leave windows unscored
        const bool detect_only = !agg && !(c->flags & RP_CTX_FULL_SCORES);
        if (!stream_encode(b, n_chunks, &in) || !stream_frames(b, *tb, in, n_chunks, &f) || !stream_levels(b, in, f, n_chunks) ||
            !stream_score_and_scan(b, sg, f, n_new, detect_only, dd, dn, max_det, det_wakeword, det_label)) return -1;
        b->chunks_seen += n_chunks;
        if (!sg.back_detections(S, max_det, det, dd, n_det, dn)) return -1;
        if (agg) {   // (one reference, or every stream's own wakeword: a batch of several wakewords was refused above)
            const DevBuf &dg = b->bank ? b->bank_agg : b->ww[0]->agg;
            if (sg.host) { if (!sg.back(agg, dg.p, S * n_new * sizeof(float))) return -1; }
            else if (!hip_ok(hipMemcpyAsync(agg, dg.p, S * n_new * sizeof(float), hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync(D2D)")) return -1;
        }
        return sg.finish() ? 0 : -1;
    });
    if (r != 0 && touched) b->poisoned = true;
    return r;
}

static const char kFiltersNeed30ms[] = "filters on a live-stream batch need 30 ms input frames: not available with the 40 ms frames of "
                                       "11.025 / 22.05 kHz input (rp_stream_batch_set_filters / rp_stream_batch_set_input)";

extern "C" {

int rp_stream_batch_new(rp_ctx *ctx, const rp_templates *t, const rp_detector_config *config, size_t S,
                        size_t max_chunks_per_call, rp_stream_batch **out) {
    if (!ctx || !t) { set_last_error("null handle"); return -1; }
    const rp_wakeword_spec one{t, nullptr, -1, 0, NAN, NAN};   // its thresholds are the config's
    return stream_batch_new(ctx, 1, &one, t->impl->dev.K, config, S, max_chunks_per_call, true, out);
}
// live-stream batches that hold several wakewords and / or a wakeword model (src/detector.rs:304-346,433-447)
int rp_stream_batch_new_multi(rp_ctx *ctx, size_t n_wakewords, const rp_wakeword_spec *wakewords, int mfcc_size,
                              const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out) {
    return stream_batch_new(ctx, n_wakewords, wakewords, mfcc_size, config, S, max_chunks_per_call, false, out);
}
// live-stream batches in which stream s holds its own wakeword bank[stream_wakeword[s]] (personal wakewords; rp_batch_detect_bank with the
// state carried between calls)
// Both constructors over a bank; sets: rp_stream_batch_new_bank_sets, rows of set_size indices per stream (else one index, set_size not read)
static int stream_batch_new_bank(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakeword, bool sets, int set_size,
                                 const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out) {
    return guarded([&]() -> int {
        const std::string name = sets ? "rp_stream_batch_new_bank_sets" : "rp_stream_batch_new_bank";
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!config || !out || !stream_wakeword) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if (sets && !set_size_ok(set_size)) return -1;
        const Bank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c) return -1;
        if (S == 0 || max_chunks_per_call == 0) { set_last_error(name + ": S and max_chunks_per_call must be >= 1"); return -1; }
        if (!bank_band_ok(bk, (int)config->band_size)) return -1;
        // before anything is allocated
        if (!batch_indices_ok(c, bk, 0, S, sets ? set_size : 0, stream_wakeword)) return -1;
        std::unique_ptr<rp_stream_batch> b(new rp_stream_batch());
        b->set_size = sets ? set_size : 0;
        b->c = c; b->bank = &bk; ++bk.live_batches; b->cfg = *config; b->S = S; b->max_chunks = max_chunks_per_call;
        // (an empty bank: no history; its mfcc_size is a placeholder -- the encode and frames stages run all the same, at the default size,
        // and nobody reads their frames.  A reserved bank declares its mfcc_size and the longest window it will ever hold, empty or not)
        b->K = (bk.dev.W || bk.ceiling) ? bk.dev.K : 5; b->max_len = bk.max_window(); b->Tmax = 1;
        if (!bank_indices_put(b.get(), 0, S, stream_wakeword)) return -1;
        if (!c->tables_for(b->K)) return -1;
        b->hist_frames = (size_t)b->max_len - 1;   // every stream keeps the history of the bank's longest window; its own starts max_len(s) - 1 frames back
        if (!stream_batch_alloc(b.get())) return -1;
        *out = b.release();
        return 0;
    });
}
int rp_stream_batch_new_bank(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakeword, const rp_detector_config *config, size_t S,
                             size_t max_chunks_per_call, rp_stream_batch **out) {
    return stream_batch_new_bank(ctx, bank, stream_wakeword, false, 0, config, S, max_chunks_per_call, out);
}
// ... in which stream s holds the SET of wakewords bank[stream_wakewords[s][0 .. set_size)] (rp_batch_detect_bank_sets with the state carried)
int rp_stream_batch_new_bank_sets(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int set_size,
                                  const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out) {
    return stream_batch_new_bank(ctx, bank, stream_wakewords, true, set_size, config, S, max_chunks_per_call, out);
}
// live-stream batches in which stream s runs its own model bank[stream_model[s]] (personal wakeword models; rp_batch_detect_model_bank with
// the state carried between calls).  Thresholds are the config's, mfcc_size is 16, the arithmetic RP_MLP_F32.
// Both constructors over a model bank; sets: rp_stream_batch_new_model_bank_sets, rows of set_size indices per stream (else one index)
static int stream_batch_new_model_bank(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_model, bool sets, int set_size,
                                       const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out) {
    return guarded([&]() -> int {
        const std::string name = sets ? "rp_stream_batch_new_model_bank_sets" : "rp_stream_batch_new_model_bank";
        if (!ctx || !bank) { set_last_error("null handle"); return -1; }
        if (!config || !out || !stream_model) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if (sets && !model_set_size_ok(set_size)) return -1;
        const ModelBank &bk = *bank->impl;
        Ctx *c = bank_call_ctx(ctx, bk.ctx);
        if (!c) return -1;
        if (S == 0 || max_chunks_per_call == 0) { set_last_error(name + ": S and max_chunks_per_call must be >= 1"); return -1; }
        // before anything is allocated
        if ((c->flags & RP_CTX_HOST_POINTERS) && !bank_indices_ok(bk.dev.W, 0, S, sets ? set_size : 0, stream_model, "model index")) return -1;
        std::unique_ptr<rp_stream_batch> b(new rp_stream_batch());
        b->set_size = sets ? set_size : 0;
        b->c = c; b->mbank = &bk; ++bk.live_batches; b->cfg = *config; b->S = S; b->max_chunks = max_chunks_per_call;
        b->K = 16; b->max_len = bk.max_window(); b->label_pitch = bk.dev.label_pitch; b->Tmax = 1;
        if (!bank_indices_put(b.get(), 0, S, stream_model)) return -1;
        if (!c->tables_for(b->K)) return -1;
        b->hist_frames = (size_t)b->max_len - 1;   // every stream keeps the history of the bank's longest window; its own starts L(s) - 1 frames back
        if (!stream_batch_alloc(b.get())) return -1;
        *out = b.release();
        return 0;
    });
}
int rp_stream_batch_new_model_bank(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_model, const rp_detector_config *config, size_t S,
                                   size_t max_chunks_per_call, rp_stream_batch **out) {
    return stream_batch_new_model_bank(ctx, bank, stream_model, false, 0, config, S, max_chunks_per_call, out);
}
// ... in which stream s holds the SET of models bank[stream_models[s][0 .. set_size)] (rp_batch_detect_model_bank_sets with the state carried)
int rp_stream_batch_new_model_bank_sets(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_models, int set_size,
                                        const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out) {
    return stream_batch_new_model_bank(ctx, bank, stream_models, true, set_size, config, S, max_chunks_per_call, out);
}
// live-stream batches over MIXED sets: stream s holds the references bank[stream_wakewords[s][..]] and the models model_bank[stream_models[s][..]]
// on one detector (rp_batch_detect_mixed_sets with the state carried)
// the two set sizes of a mixed batch: 0 .. 8 each, the text of rp_batch_detect_mixed_sets
static bool mixed_sizes_ok(int ref_set_size, int model_set_size) {
    if (ref_set_size < 0 || ref_set_size > RP_WAKEWORD_SET_MAX) {
        set_last_error("ref_set_size " + std::to_string(ref_set_size) + " is outside 0 .. " + std::to_string((int)RP_WAKEWORD_SET_MAX) + " (RP_WAKEWORD_SET_MAX)");
        return false;
    }
    if (model_set_size < 0 || model_set_size > RP_MODEL_SET_MAX) {
        set_last_error("model_set_size " + std::to_string(model_set_size) + " is outside 0 .. " + std::to_string((int)RP_MODEL_SET_MAX) + " (RP_MODEL_SET_MAX)");
        return false;
    }
    return true;
}
// both rows of streams first .. first + n - 1 in HOST arrays: every index within its bank, else an error that names stream, slot and side
static bool mixed_rows_ok(const Ctx *c, const Bank &bk, int ref_set_size, const int32_t *refs, const ModelBank &mb, int model_set_size, const int32_t *models,
                          size_t first, size_t n) {
    if (!(c->flags & RP_CTX_HOST_POINTERS)) return true;
    return (!ref_set_size || bank_indices_ok(bk.dev.W, first, n, ref_set_size, refs, "wakeword index")) &&
           (!model_set_size || bank_indices_ok(mb.dev.W, first, n, model_set_size, models, "model index"));
}
int rp_stream_batch_new_mixed_sets(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int ref_set_size,
                                   const rp_model_bank *model_bank, const int32_t *stream_models, int model_set_size, const rp_detector_config *config,
                                   size_t S, size_t max_chunks_per_call, rp_stream_batch **out) {
    return guarded([&]() -> int {
        if (!ctx || !bank || !model_bank) { set_last_error("null handle"); return -1; }
        if (!config || !out) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if (!mixed_sizes_ok(ref_set_size, model_set_size)) return -1;
        if ((ref_set_size && !stream_wakewords) || (model_set_size && !stream_models)) { set_last_error("null argument"); return -1; }
        const Bank &bk = *bank->impl;
        const ModelBank &mb = *model_bank->impl;
        Ctx *c = ctx->impl.get();
        if (bk.ctx != c) { set_last_error("the wakeword bank belongs to another context"); return -1; }
        if (mb.ctx != c) { set_last_error("the model bank belongs to another context"); return -1; }
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice")) return -1;
        if (S == 0 || max_chunks_per_call == 0) { set_last_error("rp_stream_batch_new_mixed_sets: S and max_chunks_per_call must be >= 1"); return -1; }
        // add_wakeword, src/detector.rs:316-319: a model bank is at mfcc_size 16 (an empty bank that was never reserved has a placeholder size)
        if ((bk.dev.W || bk.ceiling) && bk.dev.K != 16) { set_last_error("Usage of wakewords with different mfcc size is not supported, ignoring wakeword"); return -1; }
        if (!bank_band_ok(bk, (int)config->band_size)) return -1;
        if (config->band_size != 0 && dtw_register_tile(16, (int)config->band_size) <= 0) {
            set_last_error("rp_stream_batch_new_mixed_sets: band_size " + std::to_string((int)config->band_size) + " is not built (3..6, or 0)");
            return -1;
        }
        // before anything is allocated
        if (!mixed_rows_ok(c, bk, ref_set_size, stream_wakewords, mb, model_set_size, stream_models, 0, S)) return -1;
        std::unique_ptr<rp_stream_batch> b(new rp_stream_batch());
        b->mixed = true; b->set_size = ref_set_size; b->mset_size = model_set_size;
        b->c = c; b->bank = &bk; ++bk.live_batches; b->mbank = &mb; ++mb.live_batches; b->cfg = *config; b->S = S; b->max_chunks = max_chunks_per_call;
        // the history of the longer of the two banks' windows, reservations included: what a bank-sets batch and a model-sets batch would keep
        b->K = 16; b->max_len = std::max(bk.max_window(), mb.max_window()); b->label_pitch = mb.dev.label_pitch; b->Tmax = 1;
        if (!indices_put(b.get(), b->bank_idx, (size_t)ref_set_size, 0, S, stream_wakewords) ||
            !indices_put(b.get(), b->model_idx, (size_t)model_set_size, 0, S, stream_models)) return -1;
        if (!c->tables_for(b->K)) return -1;
        b->hist_frames = (size_t)b->max_len - 1;
        if (!stream_batch_alloc(b.get())) return -1;
        *out = b.release();
        return 0;
    });
}
// Re-target streams first_stream .. first_stream + n - 1 of such a batch: both rows removed, the new ones added in order (references, then
// models), the stream reset.  A refused row changes nothing.
int rp_stream_batch_set_mixed_sets(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *stream_wakewords, const int32_t *stream_models) {
    bool touched = false;
    const int r = guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (!b->mixed) { set_last_error("rp_stream_batch_set_mixed_sets: the batch was not made by rp_stream_batch_new_mixed_sets"); return -1; }
        if (first_stream > b->S || n > b->S - first_stream) {
            set_last_error("rp_stream_batch_set_mixed_sets: streams " + std::to_string(first_stream) + " .. " + std::to_string(first_stream) + " + " +
                           std::to_string(n) + " reach past the batch's " + std::to_string(b->S) + " streams");
            return -1;
        }
        if (n == 0) return 0;
        if ((b->set_size && !stream_wakewords) || (b->mset_size && !stream_models)) { set_last_error("null argument"); return -1; }
        // a refused index on either side leaves the batch as it was
        if (!mixed_rows_ok(c, *b->bank, b->set_size, stream_wakewords, *b->mbank, b->mset_size, stream_models, first_stream, n)) return -1;
        touched = true;
        if (!indices_put(b, b->bank_idx, (size_t)b->set_size, first_stream, n, stream_wakewords) ||
            !indices_put(b, b->model_idx, (size_t)b->mset_size, first_stream, n, stream_models)) return -1;
        return hip_ok(launch_stream_state_reset_range(c->stream, b->state.p, b->S, first_stream, n, (long long)b->fpf() * (long long)b->chunks_seen),
                      "stream_state_reset_kernel") ? 0 : -1;
    });
    if (r != 0 && touched) b->poisoned = true;
    return r;
}
void rp_stream_batch_free(rp_stream_batch *b) { delete b; }
size_t rp_stream_batch_chunks_seen(const rp_stream_batch *b) { return b ? b->chunks_seen : 0; }

int rp_stream_batch_set_input(rp_stream_batch *b, size_t sample_rate, int channels) {
    return guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, false);
        if (!c) return -1;
        if (b->chunks_seen) { set_last_error("rp_stream_batch_set_input: the streams have already received audio"); return -1; }
        if (channels < 1) { set_last_error("Unsupported channel count"); return -1; }
        size_t fi = 480, fo = 480;
        if (!resampler_frame_lengths(sample_rate, &fi, &fo)) { set_last_error("Unsupported sample rate, unable to initialize the resampler"); return -1; }
        if (b->has_filters && fo != 480) { set_last_error(kFiltersNeed30ms); return -1; }
        b->channels = channels; b->in_len = fi; b->rs = nullptr;
        if (fo != b->out_len) {  // 11.025 / 22.05 kHz: 40 ms frames of four 10 ms shifts
            b->out_len = fo;
            if (!stream_batch_alloc(b)) return -1;
        }
        if (sample_rate != 16000) {
            b->rs = c->resampler_for(sample_rate);
            if (!b->rs) return -1;
            if (!b->rs_prev[0].reserve(b->S * fi * sizeof(float)) || !b->rs_prev[1].reserve(b->S * fi * sizeof(float)) ||
                !b->rs_out.reserve(b->S * b->max_chunks * fo * sizeof(float))) return -1;
            if (!b->rs->dev.fft48 && !b->rs_xs.reserve(b->S * (1 + b->max_chunks) * fi * sizeof(float) + 64)) return -1;
            if (!hip_ok(hipMemsetAsync(b->rs_prev[0].p, 0, b->S * fi * sizeof(float), c->stream), "hipMemsetAsync")) return -1;
            b->rs_cur = 0;
        }
        return 0;
    });
}
size_t rp_stream_batch_samples_per_chunk(const rp_stream_batch *b) { return b ? b->in_len * (size_t)b->channels : 0; }

// The three filter calls; per_stream: rp_stream_batch_set_filters_bank, prepared: rp_stream_batch_set_filters_per_stream (rms_level_ref is then
// not read)
static int stream_batch_set_filters(rp_stream_batch *b, const rp_filters_config *filters, float rms_level_ref, bool per_stream, bool prepared = false) {
    return guarded([&]() -> int {
        const std::string name = prepared ? "rp_stream_batch_set_filters_per_stream" : per_stream ? "rp_stream_batch_set_filters_bank" : "rp_stream_batch_set_filters";
        if (b && !filters) { set_last_error("null argument"); return -1; }
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (b->mixed && per_stream) {
            set_last_error(name + ": a batch over mixed sets takes its level and window from several wakewords of two banks per stream; "
                                  "rp_stream_batch_set_filters_per_stream gives it the gain normaliser");
            return -1;
        }
        if (b->mixed && filters->gain_normalizer.enabled && !prepared) {
            set_last_error("rp_stream_batch_set_filters: the gain normaliser is not available on a batch over mixed sets (its window and rms_level_ref would be "
                           "per stream); the band-pass filter alone is, and rp_stream_batch_set_filters_per_stream gives every stream the gain normaliser "
                           "of its own wakewords");
            return -1;
        }
        if (prepared && !b->bank && !b->mbank) {
            set_last_error(name + ": the batch holds shared wakewords, one level and one window for every stream; rp_stream_batch_set_filters takes them");
            return -1;
        }
        if (per_stream && b->mbank) {
            set_last_error(name + ": the gain normaliser per model is not built for a batch over a model bank (a model's rms_level is not part of the "
                                  "bank); rp_stream_batch_set_filters takes the band-pass filter alone");
            return -1;
        }
        if (per_stream && !b->bank) { set_last_error(name + ": the batch was not made by rp_stream_batch_new_bank"); return -1; }
        if (per_stream && b->set_size) {
            set_last_error(name + ": the gain normaliser is not available on a batch over wakeword sets (its level and window would come from "
                                  "several wakewords per stream); rp_stream_batch_set_filters takes the band-pass filter alone");
            return -1;
        }
        if (b->chunks_seen) { set_last_error(name + ": the streams have already received audio"); return -1; }
        if (b->out_len != 480) { set_last_error(kFiltersNeed30ms); return -1; }
        const rp_gain_normalization_config &g = filters->gain_normalizer;
        if (b->mbank && g.enabled && !prepared) {
            set_last_error("rp_stream_batch_set_filters: the gain normaliser is not available on a batch over a model bank (its window and "
                           "rms_level_ref would be per stream, and a model's rms_level is not part of the bank); the band-pass filter alone is");
            return -1;
        }
        if (b->bank && g.enabled && !per_stream && !prepared) {
            set_last_error("rp_stream_batch_set_filters: the gain normaliser is not available on a batch over a wakeword bank (its window and "
                           "rms_level_ref would be per stream, stream_filters_kernel takes one value of each); the band-pass filter alone is, "
                           "and rp_stream_batch_set_filters_bank gives every stream the gain normaliser of its own wakeword");
            return -1;
        }
        // (a batch over a bank: the bank's largest window, the capacity of every stream's ring)
        const int window = std::max(b->max_len / 3, 1);   // on_wakeword_change, src/detector.rs:337; set_rms_level_ref :47
        const size_t lv = b->S * b->max_chunks * sizeof(float) + 16, st = stream_filter_state_bytes(b->S, window);
        if (!b->filt_state.reserve(st) || !b->lv_rms.reserve(lv) || !b->lv_gain.reserve(lv)) return -1;
        if (prepared && g.enabled && !b->gain_tab.reserve(gain_targets_bytes(b->S))) return -1;
        if (!hip_ok(hipMemsetAsync(b->filt_state.p, 0, st, c->stream), "hipMemsetAsync")) return -1;
        b->filt = *filters;
        b->rms_level_ref = g.enabled && g.has_gain_ref ? g.gain_ref : rms_level_ref;  // fixed_rms_level, gain_normalizer_filter.rs:56-66
        b->gain_window = window;
        b->per_stream_gain = (per_stream || prepared) && g.enabled;
        b->prep_gain = prepared && g.enabled;
        band_pass_coefficients(filters->band_pass, b->bq);
        b->has_filters = true;
        return 0;
    });
}

int rp_stream_batch_set_filters(rp_stream_batch *b, const rp_filters_config *filters, float rms_level_ref) {
    return stream_batch_set_filters(b, filters, rms_level_ref, false);
}
int rp_stream_batch_set_filters_bank(rp_stream_batch *b, const rp_filters_config *filters) {
    return stream_batch_set_filters(b, filters, NAN, true);
}

int rp_stream_batch_set_filters_per_stream(rp_stream_batch *b, const rp_filters_config *filters) {
    return stream_batch_set_filters(b, filters, NAN, false, true);
}

int rp_stream_batch_levels(rp_stream_batch *b, float *rms, float *gains) {
    return guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (!b->has_filters) { set_last_error("rp_stream_batch_levels: the batch has had no rp_stream_batch_set_filters"); return -1; }
        if (!b->levels_chunks) { set_last_error("rp_stream_batch_levels: the streams have not received audio yet"); return -1; }
        const size_t n = b->S * b->levels_chunks;
        const bool host = (c->flags & RP_CTX_HOST_POINTERS) != 0;
        const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (rms && !hip_ok(hipMemcpyAsync(rms, b->lv_rms.p, n * sizeof(float), kind, c->stream), "hipMemcpyAsync")) return -1;
        if (gains) {
            if (b->filters_on()) {
                if (!hip_ok(hipMemcpyAsync(gains, b->lv_gain.p, n * sizeof(float), kind, c->stream), "hipMemcpyAsync")) return -1;
            } else {  // both filters off: every chunk has gain 1
                std::vector<float> ones(n, 1.f);
                if (host) std::memcpy(gains, ones.data(), n * sizeof(float));
                else if (!hip_ok(hipMemcpy(gains, ones.data(), n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy")) return -1;
            }
        }
        return !host || hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize") ? 0 : -1;
    });
}

int rp_stream_batch_reset(rp_stream_batch *b, long long stream) {
    return guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (stream >= (long long)b->S) { set_last_error("rp_stream_batch_reset: no such stream"); return -1; }
        // the next chunk only refills the extractor: its three frames (3C-3 .. 3C-1) are never emitted
        return hip_ok(launch_stream_state_reset(c->stream, b->state.p, b->S, stream, (long long)b->fpf() * (long long)b->chunks_seen), "stream_state_reset_kernel") ? 0 : -1;
    });
}

// connect / disconnect of device slots: new indices for streams first_stream .. first_stream + n - 1, each reset as rp_stream_batch_reset does
// (add_wakeword on a detector without wakewords calls reset(), src/detector.rs:304-307)
// Both re-targeting calls; sets: rp_stream_batch_set_wakeword_sets, rows of set_size indices -- remove-all plus add-in-order
static int stream_batch_set_wakewords(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *wakewords, bool sets) {
    bool touched = false;
    const int r = guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (b->mixed) {
            set_last_error(std::string(sets ? "rp_stream_batch_set_wakeword_sets" : "rp_stream_batch_set_wakewords") +
                           ": the batch runs over mixed sets (rp_stream_batch_new_mixed_sets), whose streams are re-targeted with rp_stream_batch_set_mixed_sets, both rows at once");
            return -1;
        }
        if (b->mbank) {
            set_last_error(std::string(sets ? "rp_stream_batch_set_wakeword_sets" : "rp_stream_batch_set_wakewords") +
                           (b->set_size ? ": the batch runs over model sets (rp_stream_batch_new_model_bank_sets), whose streams are re-targeted with rp_stream_batch_set_model_sets"
                                        : ": the batch runs over a model bank (rp_stream_batch_new_model_bank), whose streams are re-targeted with rp_stream_batch_set_models"));
            return -1;
        }
        if (sets && !b->set_size) { set_last_error("rp_stream_batch_set_wakeword_sets: the batch was not made by rp_stream_batch_new_bank_sets"); return -1; }
        if (!b->bank) { set_last_error("rp_stream_batch_set_wakewords: the batch was not made by rp_stream_batch_new_bank"); return -1; }
        if (!sets && b->set_size) { set_last_error("rp_stream_batch_set_wakewords: the batch holds wakeword sets (rp_stream_batch_new_bank_sets); use rp_stream_batch_set_wakeword_sets"); return -1; }
        if (first_stream > b->S || n > b->S - first_stream) {
            set_last_error(std::string(sets ? "rp_stream_batch_set_wakeword_sets" : "rp_stream_batch_set_wakewords") + ": streams " + std::to_string(first_stream) + " .. " + std::to_string(first_stream) + " + " +
                           std::to_string(n) + " reach past the batch's " + std::to_string(b->S) + " streams");
            return -1;
        }
        if (n == 0) return 0;
        if (!wakewords) { set_last_error("null argument"); return -1; }
        // a refused index leaves the batch as it was
        if (!batch_indices_ok(c, *b->bank, first_stream, n, b->set_size, wakewords)) return -1;
        touched = true;
        if (!bank_indices_put(b, first_stream, n, wakewords)) return -1;
        return hip_ok(launch_stream_state_reset_range(c->stream, b->state.p, b->S, first_stream, n, (long long)b->fpf() * (long long)b->chunks_seen),
                      "stream_state_reset_kernel") ? 0 : -1;
    });
    if (r != 0 && touched) b->poisoned = true;
    return r;
}

int rp_stream_batch_set_wakewords(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *wakewords) {
    return stream_batch_set_wakewords(b, first_stream, n, wakewords, false);
}
int rp_stream_batch_set_wakeword_sets(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *stream_wakewords) {
    return stream_batch_set_wakewords(b, first_stream, n, stream_wakewords, true);
}

// connect / disconnect / retarget slots of a batch over a model bank: as rp_stream_batch_set_wakewords, each touched stream reset
// Both re-targeting calls; sets: rp_stream_batch_set_model_sets, rows of set_size indices -- remove-all plus add-in-order
static int stream_batch_set_models(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *models, bool sets) {
    bool touched = false;
    const int r = guarded([&]() -> int {
        const std::string name = sets ? "rp_stream_batch_set_model_sets" : "rp_stream_batch_set_models";
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (b->mixed) {
            set_last_error(name + ": the batch runs over mixed sets (rp_stream_batch_new_mixed_sets), whose streams are re-targeted with rp_stream_batch_set_mixed_sets, both rows at once");
            return -1;
        }
        if (sets && !(b->mbank && b->set_size)) { set_last_error(name + ": the batch was not made by rp_stream_batch_new_model_bank_sets"); return -1; }
        if (!b->mbank) { set_last_error(name + ": the batch was not made by rp_stream_batch_new_model_bank"); return -1; }
        if (!sets && b->set_size) { set_last_error(name + ": the batch holds model sets (rp_stream_batch_new_model_bank_sets); use rp_stream_batch_set_model_sets"); return -1; }
        if (first_stream > b->S || n > b->S - first_stream) {
            set_last_error(name + ": streams " + std::to_string(first_stream) + " .. " + std::to_string(first_stream) + " + " +
                           std::to_string(n) + " reach past the batch's " + std::to_string(b->S) + " streams");
            return -1;
        }
        if (n == 0) return 0;
        if (!models) { set_last_error("null argument"); return -1; }
        // a refused index leaves the batch as it was
        if ((c->flags & RP_CTX_HOST_POINTERS) && !bank_indices_ok(b->mbank->dev.W, first_stream, n, b->set_size, models, "model index")) return -1;
        touched = true;
        if (!bank_indices_put(b, first_stream, n, models)) return -1;
        return hip_ok(launch_stream_state_reset_range(c->stream, b->state.p, b->S, first_stream, n, (long long)b->fpf() * (long long)b->chunks_seen),
                      "stream_state_reset_kernel") ? 0 : -1;
    });
    if (r != 0 && touched) b->poisoned = true;
    return r;
}
int rp_stream_batch_set_models(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *models) {
    return stream_batch_set_models(b, first_stream, n, models, false);
}
int rp_stream_batch_set_model_sets(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *stream_models) {
    return stream_batch_set_models(b, first_stream, n, stream_models, true);
}

// the logits of the last process call of a batch over a model bank, [S][frames of that call][rp_model_bank_labels(bank, -1)]; a batch over
// model sets: [S][set_size][frames of that call][..]
int rp_stream_batch_logits(rp_stream_batch *b, float *logits) {
    return guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (!b->mbank) { set_last_error("rp_stream_batch_logits: the batch was not made by rp_stream_batch_new_model_bank"); return -1; }
        if (!b->logit_frames) { set_last_error("rp_stream_batch_logits: the streams have not received audio yet"); return -1; }
        const size_t bytes = b->S * (b->mixed ? (size_t)b->mset_size : b->slots()) * b->logit_frames * (size_t)b->label_pitch * sizeof(float);
        if (bytes == 0) return 0;   // an empty bank has no labels
        if (!logits) { set_last_error("null argument"); return -1; }
        const bool host = (c->flags & RP_CTX_HOST_POINTERS) != 0;
        if (!hip_ok(hipMemcpyAsync(logits, b->logits.p, bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream), "hipMemcpyAsync")) return -1;
        return !host || hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize") ? 0 : -1;
    });
}

int rp_stream_batch_slot_scores(rp_stream_batch *b, float *agg, float *avg) {
    return guarded([&]() -> int {
        Ctx *c = stream_batch_enter(b, true);
        if (!c) return -1;
        if (!b->mixed) {   // (a batch over mixed sets: the reference slots' rows; the model slots' per-window output is rp_stream_batch_logits)
            if (b->mbank && b->set_size) { set_last_error("rp_stream_batch_slot_scores: a batch over model sets keeps no aggregate per slot; rp_stream_batch_logits returns its per-slot, per-window output"); return -1; }
            if (b->mbank) { set_last_error("rp_stream_batch_slot_scores: a batch over a model bank has one model per stream and no slots; rp_stream_batch_logits returns its per-window output"); return -1; }
            if (!b->set_size) { set_last_error("rp_stream_batch_slot_scores: the batch was not made by rp_stream_batch_new_bank_sets"); return -1; }
        }
        if (!b->slot_frames) { set_last_error("rp_stream_batch_slot_scores: the streams have not received audio yet"); return -1; }
        const size_t bytes = b->S * (size_t)b->set_size * b->slot_frames * sizeof(float);   // 0: a mixed batch without a reference side
        const bool host = (c->flags & RP_CTX_HOST_POINTERS) != 0;
        const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (bytes && agg && !hip_ok(hipMemcpyAsync(agg, b->bank_agg.p, bytes, kind, c->stream), "hipMemcpyAsync")) return -1;
        if (bytes && avg && !hip_ok(hipMemcpyAsync(avg, b->bank_avg.p, bytes, kind, c->stream), "hipMemcpyAsync")) return -1;
        return !host || hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize") ? 0 : -1;
    });
}

int rp_stream_batch_process(rp_stream_batch *b, const void *pcm, rp_sample_format fmt, size_t n_chunks, size_t pcm_stride,
                            rp_batch_detection *det, int32_t *n_det, int max_det, float *agg) {
    return stream_batch_process(b, pcm, fmt, n_chunks, pcm_stride, det, n_det, max_det, agg, nullptr, nullptr);
}
int rp_stream_batch_process_multi(rp_stream_batch *b, const void *pcm, rp_sample_format fmt, size_t n_chunks, size_t pcm_stride,
                                  rp_batch_detection *det, int32_t *det_wakeword, int32_t *det_label, int32_t *n_det, int max_det) {
    return stream_batch_process(b, pcm, fmt, n_chunks, pcm_stride, det, n_det, max_det, nullptr, det_wakeword, det_label);
}

}  // extern "C"
