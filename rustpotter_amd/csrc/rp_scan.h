// rp_scan.h -- what the scan kernels share (rp_scan.hip, rp_scan_sets.hip): the carried lane state, the detections' output block, a window's
// proposal, bank_lane, the slots of a set, scan_frames -- the one copy of the detection state machine -- and the two frames around it,
// scan_recording and scan_live.  Device code only; include behind rp_device.h.
#pragma once
#include "rp_device.h"

#include <cstddef>

namespace rp {

// ------------------------------------------------------------------------- lane state
// The detector state of one stream: the countdown / partial detection / window bookkeeping (src/detector.rs:62-79) in absolute frame
// numbers, and the VadDetector's scalars (its window lies in LDS while a kernel runs).  A whole-recording kernel starts from a fresh one;
// a live stream carries it between rp_stream_batch_process calls as the head of its StreamState.
struct ScanLane {
    long long win_start, resume;
    int has_partial, p_counter, countdown, vad_index, voice_countdown;
    int p_ww;        // wakeword the partial detection belongs to (detectors that hold several)
    int p_label;     // its label index when that wakeword is a model, else -1
    int pad;
    long long p_window;
    float p_score, p_avg;
};
struct StreamState {
    ScanLane lane;
    float vad_window[50];
};
static_assert(sizeof(ScanLane) == 64 && sizeof(StreamState) == 264, "the carried state: a 64-byte head and the VAD window");

// Rustpotter::reset (src/detector.rs:290-302) without the VAD window: no partial detection, an empty VAD, the next chunk only refills the
// extractor, so the next frame seen is `resume`
__device__ __forceinline__ void lane_reset(ScanLane &z, long long resume) {
    z.win_start = z.resume = resume;
    z.has_partial = 0; z.p_counter = 0; z.countdown = 0; z.vad_index = 0; z.voice_countdown = 0;
}
__device__ __forceinline__ ScanLane fresh_lane() {
    ScanLane z;
    lane_reset(z, 0);
    z.p_ww = 0; z.p_label = -1; z.pad = 0;
    z.p_window = 0; z.p_score = 0.f; z.p_avg = 0.f;
    return z;
}

// ------------------------------------------------------------------------- output
// The detections of a call, [S][max_det] with n_det [S]; det_ww / det_label (optional) are int32 columns beside det.
struct ScanOut {
    BatchDetection *det;
    int32_t *det_ww, *det_label, *n_det;
    int max_det;
    // detection number nd of stream s, dropped when the stream's slots are full
    __device__ __forceinline__ void put(size_t s, int nd, int32_t stream, long long f, const ScanLane &z, int32_t ww, int32_t label) const {
        if (nd >= max_det) return;
        BatchDetection d;
        d.stream = stream; d.frame = (int32_t)f; d.window = (int32_t)z.p_window; d.counter = z.p_counter;
        d.avg_score = z.p_avg; d.score = z.p_score;
        const size_t slot = s * (size_t)max_det + nd;
        det[slot] = d;
        if (det_ww) det_ww[slot] = ww;
        if (det_label) det_label[slot] = label;
    }
    // slots behind the detections a stream reports are zeroed (label -1, "no label"): the output block is a function of the input alone
    __device__ __forceinline__ void finish(size_t s, int nd) const {
        n_det[s] = nd;
        for (int i = nd; i < max_det; ++i) {
            det[s * (size_t)max_det + i] = BatchDetection{};
            if (det_ww) det_ww[s * (size_t)max_det + i] = 0;
            if (det_label) det_label[s * (size_t)max_det + i] = -1;
        }
    }
};

// ------------------------------------------------------------------------- proposals
// What the wakewords of a lane say about one window: `found` when one proposes a detection
struct Proposal {
    bool found;
    float score, avg;
    int ww, label;   // the proposing wakeword and its label for this window (-1: not a model)
};
// How a stream that holds the one wakeword bank[wi] runs the state machine, as a `Rustpotter` with that wakeword alone: its window length
// (max_mfcc_frames; the countdown is max_len / 2), its own thresholds over the config's, the avg test only when it has an averaged template
// and the effective avg_threshold != 0 (wakeword_comp.rs:85).  none: wi is outside the bank, the stream has no wakeword.
struct BankLane {
    bool none, avg_on;
    int max_len;
    float thr, athr;
};
__device__ __forceinline__ BankLane bank_lane(const BankDev &b, int wi, const ScanConfig &cfg) {
    BankLane r{true, false, 0, 0.f, 0.f};
    if (wi < 0 || wi >= b.W) return r;
    const float own_thr = b.ww[wi].threshold, own_athr = b.ww[wi].avg_threshold;
    r.none = false;
    r.max_len = b.ww[wi].max_len;
    r.thr = own_thr == own_thr ? own_thr : cfg.threshold;   // NaN: the wakeword has none of its own
    r.athr = own_athr == own_athr ? own_athr : cfg.avg_threshold;
    r.avg_on = b.ww[wi].avg >= 0 && r.athr != 0.f;
    return r;
}

// on_wakeword_change, src/detector.rs:328-334: the window of a detector is as long as its longest wakeword; 0: no live slot
__device__ __forceinline__ int set_max_len(const BankDev &b, const int32_t *__restrict__ set, int set_size) {
    int lmax = 0;
    for (int j = 0; j < set_size; ++j) {
        const int wi = set[j];
        if (wi >= 0 && wi < b.W) lmax = max(lmax, b.ww[wi].max_len);
    }
    return lmax;
}

// ------------------------------------------------------------------------- the slots of a live set
// A live kernel keeps the slots of its stream's set in registers: every loop over them is unrolled to the limit of a set.
// Reference slots: wi[j] as given, r[j] = bank_lane (none: an empty slot); model slots: mi[j], -1 for an empty slot (b: ModelBank::scan).
// Both return the longest window over the live slots, 0: none is live.
__device__ __forceinline__ int load_ref_slots(const BankDev &b, const int32_t *__restrict__ set, int set_size, const ScanConfig &cfg,
                                              int (&wi)[kScanMaxWakewords], BankLane (&r)[kScanMaxWakewords]) {
    int max_len = 0;
#pragma unroll
    for (int j = 0; j < kScanMaxWakewords; ++j) {
        wi[j] = j < set_size ? set[j] : -1;
        r[j] = bank_lane(b, wi[j], cfg);
        max_len = max(max_len, r[j].max_len);
    }
    return max_len;
}
__device__ __forceinline__ int load_model_slots(const BankDev &b, const int32_t *__restrict__ set, int set_size, int (&mi)[kScanMaxWakewords]) {
    int max_len = 0;
#pragma unroll
    for (int j = 0; j < kScanMaxWakewords; ++j) {
        mi[j] = j < set_size ? set[j] : -1;
        if (mi[j] < 0 || mi[j] >= b.W) mi[j] = -1;
        else max_len = max(max_len, b.ww[mi[j]].max_len);
    }
    return max_len;
}
// What the slots say about new frame i, folded into p (ww < 0: nobody has proposed yet): the best score wins, the first slot of equals --
// propose_best's rule (run_wakeword_detectors, src/detector.rs:433-447) with the bank index as the wakeword.  rows: the stream's
// [set_size][n_new].  A reference slot proposes with its own thresholds (>), a model slot where its score is not -2:
// nn_score_set_stream_kernel applied its gates (>=); its window's label travels with the proposal.
__device__ __forceinline__ void propose_ref_slots(Proposal &p, const int (&wi)[kScanMaxWakewords], const BankLane (&r)[kScanMaxWakewords],
                                                  const float *__restrict__ agg, const float *__restrict__ avg, size_t row0, int n_new, int i) {
#pragma unroll
    for (int j = 0; j < kScanMaxWakewords; ++j) {
        if (r[j].none) continue;
        const size_t row = row0 + (size_t)j * (size_t)n_new + i;
        const float sj = agg[row];
        float aj = 0.f;
        bool pass = true;
        if (r[j].avg_on) { aj = avg[row]; pass = !(aj < r[j].athr); }
        if (pass && sj > r[j].thr && (p.ww < 0 || sj > p.score)) { p.ww = wi[j]; p.score = sj; p.avg = aj; }
    }
}
__device__ __forceinline__ void propose_model_slots(Proposal &p, const int (&mi)[kScanMaxWakewords], const float *__restrict__ agg,
                                                    const float *__restrict__ avg, const int32_t *__restrict__ label, size_t row0, int n_new, int i) {
#pragma unroll
    for (int j = 0; j < kScanMaxWakewords; ++j) {
        if (mi[j] < 0) continue;
        const size_t row = row0 + (size_t)j * (size_t)n_new + i;
        const float sj = agg[row];
        if (sj != -2.f && (p.ww < 0 || sj > p.score)) { p.ww = mi[j]; p.score = sj; p.avg = avg[row]; p.label = label[row]; }
    }
}

// ------------------------------------------------------------------------- the state machine
// The partial-detection / countdown state machine of src/detector.rs:377-454 with reset() of :290-302 for one lane, over the frames
// f0 .. f0+n-1 (i = 0 .. n-1; vv[i] is frame f0+i's VAD value, vwin[.][lane] the lane's VadDetector::window).  propose(f, i) is what the
// lane's wakewords say about the window of max_len frames that ends at frame f, emit(nd, f, z) reports detection number nd of this call.
// Returns the detections emitted.
// Frame f is emitted while chunk c = f/3 + 1 is processed; after an emit the extractor and the window are cleared, the rest of that
// chunk's frames are dropped (find_map, :372-375), chunk c+1 only refills the extractor, so the next frame seen is 3*(f/3) + 6.  In
// general, with fpf frames per input frame (4 behind the 11.025 / 22.05 kHz resampler): frame f's last shift f+3 lies in chunk
// c = (f+3)/fpf, the refill starts with shift fpf*(c+1) and its fourth shift completes frame fpf*(c+1).
template <class Propose, class Emit>
__device__ __forceinline__ int scan_frames(ScanLane &z, float (*vwin)[64], int lane, const float *__restrict__ vv, float vad_mode_value,
                                           long long f0, int n, int max_len, const ScanConfig &cfg, Propose propose, Emit emit) {
    int nd = 0;
    for (int i = 0; i < n; ++i) {
        const long long f = f0 + i;
        if (f < 0 || f < z.resume) continue;  // frames the extractor never emits (first chunk of a live stream, refill after a reset)
        // process_new_mfccs :379-383: the VAD only sees a frame while no partial detection exists (VadDetector, src/mfcc/vad.rs:3-50)
        bool should_run = true;
        if (vv && !z.has_partial) {
            vwin[z.vad_index][lane] = vv[i];
            z.vad_index = z.vad_index >= 49 ? 0 : z.vad_index + 1;
            float mn = RP_INF;
            for (int j = 0; j < 50; ++j) { float w = vwin[j][lane]; if (w == w && w < mn) mn = w; }
            mn = fmaxf(mn, 0.01f);
            const float th = mn * vad_mode_value;
            int n_high = 0;
            for (int j = 0; j < 50; ++j) n_high += vwin[j][lane] > th ? 1 : 0;
            if (n_high > 10) z.voice_countdown = 500;
            if (z.voice_countdown > 0) { z.voice_countdown -= 1; should_run = true; } else should_run = false;
        }
        if (f - z.win_start + 1 < max_len) continue;
        if (!should_run) continue;
        if (z.countdown != 0) z.countdown -= 1;
        if (z.has_partial) {
            const bool done = z.countdown == 0 ? true : (cfg.eager && z.p_counter >= cfg.min_scores);
            if (done) {
                z.has_partial = 0;  // take()
                if (z.p_counter >= cfg.min_scores) {
                    emit(nd, f, z);
                    ++nd;
                    lane_reset(z, cfg.fpf * ((f + 3) / cfg.fpf + 1));
                    if (vv)
                        for (int j = 0; j < 50; ++j) vwin[j][lane] = __builtin_nanf("");
                    continue;
                }
            }
        }
        const Proposal p = propose(f, i);
        if (p.found) {
            const int counter = z.has_partial ? z.p_counter + 1 : 1;
            if (!z.has_partial || z.p_score < p.score) {
                z.p_score = p.score; z.p_avg = p.avg; z.p_window = f - max_len + 1; z.has_partial = 1;
                z.p_ww = p.ww; z.p_label = p.label;
            }
            z.p_counter = counter;
            z.countdown = (int)(max_len / 2);
        }
    }
    return nd;
}
// The live kernels run scan_frames over the n_new frames of this call with the stream's carried state.  Frame i of the call is absolute
// frame f0 + i; the window ending at it is row i of the stream's agg / avg (the history prefix is max_len-1 frames long).  The 64-byte
// head of the state travels every call, the 200 bytes of the VAD window only in detectors that have a VAD (as one struct copy each way a
// call moved 34 MB in 264-byte strides for 65 536 streams: 0.019 of a 0.32 ms live call).
__device__ __forceinline__ void stream_state_load(const StreamState *sp, ScanLane &z, float (*vwin)[64], int lane, bool vad) {
    __builtin_memcpy(&z, &sp->lane, sizeof(ScanLane));
    if (vad)
        for (int i = 0; i < 50; ++i) vwin[i][lane] = sp->vad_window[i];
}
__device__ __forceinline__ void stream_state_store(StreamState *sp, const ScanLane &z, float (*vwin)[64], int lane, bool vad) {
    if (vad)
        for (int i = 0; i < 50; ++i) sp->vad_window[i] = vwin[i][lane];
    __builtin_memcpy(&sp->lane, &z, sizeof(ScanLane));
}

// ------------------------------------------------------------------------- the two frames
// Whole recordings: stream s (this lane) from a fresh state over frames 0 .. n_frames - 1, its window max_len frames long.  hot (optional):
// the flag the scoring pass raised for a stream with a window that can fire, put back to 0 here (Ctx::hot_flags); a stream without it, one
// that is not live (no wakeword, no live slot) and one with fewer frames than its window report nothing.
template <class Propose, class Emit>
__device__ __forceinline__ void scan_recording(float (*vwin)[64], int lane, size_t s, uint32_t *__restrict__ hot, int max_len, bool live,
                                               const float *__restrict__ vad_value, float vad_mode_value, size_t n_frames, const ScanConfig &cfg,
                                               const ScanOut &out, Propose propose, Emit emit) {
    bool candidate = true;
    if (hot) {
        candidate = hot[s] != 0u;
        if (candidate) hot[s] = 0u;   // consumed
    }
    if (!live || !candidate || n_frames < (size_t)max_len) { out.finish(s, 0); return; }
    const float *vv = vad_value ? vad_value + s * n_frames : nullptr;
    if (vv)
        for (int i = 0; i < 50; ++i) vwin[i][lane] = __builtin_nanf("");
    ScanLane z = fresh_lane();
    out.finish(s, scan_frames(z, vwin, lane, vv, vad_mode_value, 0, (int)n_frames, max_len, cfg, propose, emit));
}
// Live: the n_new frames of this call with the carried state of stream s (this lane); vad_value [S][n_new].  A stream that is not live
// reports nothing and keeps its state as it is (re-targeting a stream resets it).
template <class Propose, class Emit>
__device__ __forceinline__ void scan_live(float (*vwin)[64], int lane, size_t s, int max_len, bool live, const float *__restrict__ vad_value,
                                          float vad_mode_value, long long f0, int n_new, const ScanConfig &cfg, StreamState *__restrict__ state,
                                          const ScanOut &out, Propose propose, Emit emit) {
    int nd = 0;
    if (live) {
        const float *vv = vad_value ? vad_value + s * (size_t)n_new : nullptr;
        ScanLane z;
        stream_state_load(state + s, z, vwin, lane, vv != nullptr);
        nd = scan_frames(z, vwin, lane, vv, vad_mode_value, f0, n_new, max_len, cfg, propose, emit);
        stream_state_store(state + s, z, vwin, lane, vv != nullptr);
    }
    out.finish(s, nd);
}

}  // namespace rp
