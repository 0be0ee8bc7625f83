// rp_scan_sets.hip -- the detection state machine (scan_frames, rp_scan.h) for streams that hold a SET: a `Rustpotter` with several
// add_wakeword calls (src/detector.rs:304-346,433-447) -- wakeword references of a wakeword bank (scan_set_*), models of a model bank
// (scan_model_set_*), or both on one detector (scan_mixed_set_*).  Each kind has a whole-recording kernel over the proposal rows the scoring
// pass folded (dtw_set_kernel, nn_score_model_set_kernel) and a live kernel over the slot rows of this call (dtw_set_stream_kernel /
// dtw_mixed_stream_kernel, nn_score_set_stream_kernel), the state carried.  They are fronts of scan_recording / scan_live (rp_scan.h):
// a front finds the stream's window length Lmax(s) and says how a window's proposal is read.
// For a model bank, b is its scan entries (ModelBank::scan: max_len = train_size).  A detection names the winner's index in ITS OWN bank and,
// for a model, its label (-1 for a reference).
#include "rp_device.h"
#include "rp_scan.h"

namespace rp {

// ------------------------------------------------------------------------- whole recordings
// The window length (and the countdown, Lmax(s) / 2) comes from the stream's set, the proposal of a window from the three rows
// dtw_set_kernel folded -- best_ww < 0: nobody proposes.
__global__ __launch_bounds__(64) void scan_set_kernel(BankDev b, const int32_t *__restrict__ stream_wakewords, int set_size,
                                                      const float *__restrict__ best, const float *__restrict__ best_avg,
                                                      const int32_t *__restrict__ best_ww, size_t win_pitch,
                                                      const float *__restrict__ vad_value, float vad_mode_value, size_t S, size_t n_frames,
                                                      ScanConfig cfg, BatchDetection *__restrict__ det, int32_t *__restrict__ det_ww,
                                                      int32_t *__restrict__ n_det, int max_det, uint32_t *__restrict__ hot) {
    __shared__ float vwin[50][64];  // VadDetector::window, one column per stream (lane)
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    // (this one kernel keeps the frame's text in place: through scan_recording its call measured 0.06 ms in 15.1 ms slower than before,
    // just outside the run-to-run spread -- profiles/live_lane_fold.txt)
    bool candidate = true;
    if (hot) {
        candidate = hot[s] != 0u;
        if (candidate) hot[s] = 0u;   // consumed (Ctx::hot_flags)
    }
    const int max_len = set_max_len(b, stream_wakewords + s * (size_t)set_size, set_size);
    const ScanOut out{det, det_ww, nullptr, n_det, max_det};
    if (max_len == 0 || !candidate || n_frames < (size_t)max_len) { out.finish(s, 0); return; }
    const size_t row0 = s * win_pitch;
    const float *vv = vad_value ? vad_value + s * n_frames : nullptr;
    if (vv)
        for (int i = 0; i < 50; ++i) vwin[i][lane] = __builtin_nanf("");
    ScanLane z = fresh_lane();
    const int nd = scan_frames(
        z, vwin, lane, vv, vad_mode_value, 0, (int)n_frames, max_len, cfg,
        [&](long long f, int) {
            const size_t row = row0 + (size_t)(f - max_len + 1);
            const int ww = best_ww[row];
            return Proposal{ww >= 0, best[row], best_avg[row], ww, -1};
        },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s + cfg.stream_base, f, z, z.p_ww, -1); });
    out.finish(s, nd);
}

// ... the four rows nn_score_model_set_kernel folded: the proposal carries the winner's label
__global__ __launch_bounds__(64) void scan_model_set_kernel(BankDev b, const int32_t *__restrict__ stream_models, int set_size,
                                                            const float *__restrict__ best, const float *__restrict__ best_avg,
                                                            const int32_t *__restrict__ best_ww, const int32_t *__restrict__ best_label,
                                                            size_t win_pitch, const float *__restrict__ vad_value, float vad_mode_value, size_t S,
                                                            size_t n_frames, ScanConfig cfg, BatchDetection *__restrict__ det,
                                                            int32_t *__restrict__ det_ww, int32_t *__restrict__ det_label,
                                                            int32_t *__restrict__ n_det, int max_det, uint32_t *__restrict__ hot) {
    __shared__ float vwin[50][64];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const int max_len = set_max_len(b, stream_models + s * (size_t)set_size, set_size);
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    const size_t row0 = s * win_pitch;
    scan_recording(
        vwin, lane, s, hot, max_len, max_len > 0, vad_value, vad_mode_value, n_frames, cfg, out,
        [&](long long f, int) {
            const size_t row = row0 + (size_t)(f - max_len + 1);
            const int ww = best_ww[row];
            return Proposal{ww >= 0, best[row], best_avg[row], ww, best_label[row]};
        },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s + cfg.stream_base, f, z, z.p_ww, z.p_label); });
}

// ... both kinds.  The window of stream s is Lmax(s) frames, the longest over the live slots of both rows (table[s].max_len,
// stream_targets_kernel).  Either side's proposal rows were written for that side's own, shorter or equal, window: the window that starts
// at frame w is scored from frame w whatever Lmax is, so the rows are read as they are and only the windows f - Lmax(s) + 1 count.  Per
// window the better passing proposal wins, the reference of equals (references are added before models).  A side without a live slot
// for the stream is not read.
__global__ __launch_bounds__(64) void scan_mixed_set_kernel(MixedProposals refs, MixedProposals models, const BankWakeword *__restrict__ table,
                                                            size_t win_pitch, const float *__restrict__ vad_value, float vad_mode_value, size_t S,
                                                            size_t n_frames, ScanConfig cfg, BatchDetection *__restrict__ det,
                                                            int32_t *__restrict__ det_ww, int32_t *__restrict__ det_label,
                                                            int32_t *__restrict__ n_det, int max_det, uint32_t *__restrict__ hot) {
    __shared__ float vwin[50][64];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const bool ref_live = refs.set_size > 0 && set_max_len(refs.bank, refs.rows + s * (size_t)refs.set_size, refs.set_size) > 0;
    const bool model_live = models.set_size > 0 && set_max_len(models.bank, models.rows + s * (size_t)models.set_size, models.set_size) > 0;
    const int max_len = table[s].max_len;
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    const size_t row0 = s * win_pitch;
    scan_recording(
        vwin, lane, s, hot, max_len, max_len > 0 && (ref_live || model_live), vad_value, vad_mode_value, n_frames, cfg, out,
        [&](long long f, int) {
            const size_t row = row0 + (size_t)(f - max_len + 1);
            Proposal p{false, 0.f, 0.f, -1, -1};
            if (ref_live) {
                const int ww = refs.best_ww[row];
                if (ww >= 0) p = Proposal{true, refs.best[row], refs.best_avg[row], ww, -1};
            }
            if (model_live) {
                const int ww = models.best_ww[row];
                if (ww >= 0) {
                    const float sm = models.best[row];
                    if (!p.found || sm > p.score) p = Proposal{true, sm, models.best_avg[row], ww, models.best_label[row]};
                }
            }
            return p;
        },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s + cfg.stream_base, f, z, z.p_ww, z.p_label); });
}

hipError_t launch_scan_set(hipStream_t st, const BankDev &b, const int32_t *stream_wakewords, int set_size, const float *best, const float *best_avg,
                           const int32_t *best_ww, size_t win_pitch, const float *vad_value, float vad_mode_value, size_t S, size_t n_frames,
                           const ScanConfig &cfg, BatchDetection *det, int32_t *det_ww, int32_t *n_det, int max_det, uint32_t *hot) {
    if (S == 0) return hipSuccess;
    if (n_frames > 0x7fffffffULL || set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;   // a detection's frame is an int32
    hipLaunchKernelGGL(scan_set_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, b, stream_wakewords, set_size, best, best_avg, best_ww,
                       win_pitch, vad_value, vad_mode_value, S, n_frames, cfg, det, det_ww, n_det, max_det, hot);
    return hipGetLastError();
}

hipError_t launch_scan_model_set(hipStream_t st, const BankDev &b, const int32_t *stream_models, int set_size, const float *best,
                                 const float *best_avg, const int32_t *best_ww, const int32_t *best_label, size_t win_pitch, const float *vad_value,
                                 float vad_mode_value, size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det, int32_t *det_ww,
                                 int32_t *det_label, int32_t *n_det, int max_det, uint32_t *hot) {
    if (S == 0) return hipSuccess;
    if (n_frames > 0x7fffffffULL || set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;   // a detection's frame is an int32
    hipLaunchKernelGGL(scan_model_set_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, b, stream_models, set_size, best, best_avg, best_ww,
                       best_label, win_pitch, vad_value, vad_mode_value, S, n_frames, cfg, det, det_ww, det_label, n_det, max_det, hot);
    return hipGetLastError();
}

hipError_t launch_scan_mixed_set(hipStream_t st, const MixedProposals &refs, const MixedProposals &models, const BankWakeword *table, size_t win_pitch,
                                 const float *vad_value, float vad_mode_value, size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det,
                                 int32_t *det_ww, int32_t *det_label, int32_t *n_det, int max_det, uint32_t *hot) {
    if (S == 0) return hipSuccess;
    if (n_frames > 0x7fffffffULL || !table) return hipErrorInvalidValue;   // a detection's frame is an int32
    for (const MixedProposals *m : {&refs, &models}) {
        if (m->set_size < 0 || m->set_size > kScanMaxWakewords) return hipErrorInvalidValue;
        if (m->set_size && (!m->rows || !m->best || !m->best_avg || !m->best_ww)) return hipErrorInvalidValue;
    }
    if (models.set_size && !models.best_label) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_mixed_set_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, refs, models, table, win_pitch, vad_value,
                       vad_mode_value, S, n_frames, cfg, det, det_ww, det_label, n_det, max_det, hot);
    return hipGetLastError();
}

// ------------------------------------------------------------------------- live
// Slot rows [S][set_size][n_new]; per frame every live slot proposes (propose_ref_slots / propose_model_slots, rp_scan.h).  Window length,
// countdown and every threshold are read from the bank in this call.  The proposing window's wakeword and label travel in the stream's
// state (p_ww, p_label), so a detection an earlier call's window won reports its index and label.
__global__ __launch_bounds__(64) void scan_set_stream_kernel(BankDev b, const int32_t *__restrict__ stream_wakewords, int set_size,
                                                             const float *__restrict__ agg, const float *__restrict__ avg,
                                                             const float *__restrict__ vad_value, float vad_mode_value, size_t S, long long f0,
                                                             int n_new, ScanConfig cfg, StreamState *__restrict__ state,
                                                             BatchDetection *__restrict__ det, int32_t *__restrict__ det_ww,
                                                             int32_t *__restrict__ det_label, int32_t *__restrict__ n_det, int max_det) {
    __shared__ float vwin[50][64];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    int wi[kScanMaxWakewords];
    BankLane r[kScanMaxWakewords];
    const int max_len = load_ref_slots(b, stream_wakewords + s * (size_t)set_size, set_size, cfg, wi, r);
    const size_t row0 = s * (size_t)set_size * (size_t)n_new;
    scan_live(
        vwin, lane, s, max_len, max_len > 0, vad_value, vad_mode_value, f0, n_new, cfg, state, out,
        [&](long long, int i) {
            Proposal p{false, 0.f, 0.f, -1, -1};
            propose_ref_slots(p, wi, r, agg, avg, row0, n_new, i);
            p.found = p.ww >= 0;
            return p;
        },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s, f, z, z.p_ww, -1); });
}

__global__ __launch_bounds__(64) void scan_model_set_stream_kernel(BankDev b, const int32_t *__restrict__ stream_models, int set_size,
                                                                   const float *__restrict__ agg, const float *__restrict__ avg,
                                                                   const int32_t *__restrict__ label, const float *__restrict__ vad_value,
                                                                   float vad_mode_value, size_t S, long long f0, int n_new, ScanConfig cfg,
                                                                   StreamState *__restrict__ state, BatchDetection *__restrict__ det,
                                                                   int32_t *__restrict__ det_ww, int32_t *__restrict__ det_label,
                                                                   int32_t *__restrict__ n_det, int max_det) {
    __shared__ float vwin[50][64];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    int mi[kScanMaxWakewords];
    const int max_len = load_model_slots(b, stream_models + s * (size_t)set_size, set_size, mi);
    const size_t row0 = s * (size_t)set_size * (size_t)n_new;
    scan_live(
        vwin, lane, s, max_len, max_len > 0, vad_value, vad_mode_value, f0, n_new, cfg, state, out,
        [&](long long, int i) {
            Proposal p{false, 0.f, 0.f, -1, -1};
            propose_model_slots(p, mi, agg, avg, label, row0, n_new, i);
            p.found = p.ww >= 0;
            return p;
        },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s, f, z, z.p_ww, z.p_label); });
}

// Both kinds: ragg / ravg [S][ref set][n_new] of dtw_mixed_stream_kernel, magg / mavg / mlabel [S][model set][n_new] of
// nn_score_set_stream_kernel; the first of equals in add_wakeword's order: reference slots, then model slots.  Window length and countdown
// are Lmax(s) of the table, prepared in this call.  The kind of a carried partial detection travels in p_label (-1: a reference; a passing
// model window always has a label).
__global__ __launch_bounds__(64) void scan_mixed_set_stream_kernel(BankDev rb, const int32_t *__restrict__ ref_rows, int ref_size, BankDev mb,
                                                                   const int32_t *__restrict__ model_rows, int model_size,
                                                                   const BankWakeword *__restrict__ table, const float *__restrict__ ragg,
                                                                   const float *__restrict__ ravg, const float *__restrict__ magg,
                                                                   const float *__restrict__ mavg, const int32_t *__restrict__ mlabel,
                                                                   const float *__restrict__ vad_value, float vad_mode_value, size_t S, long long f0,
                                                                   int n_new, ScanConfig cfg, StreamState *__restrict__ state,
                                                                   BatchDetection *__restrict__ det, int32_t *__restrict__ det_ww,
                                                                   int32_t *__restrict__ det_label, int32_t *__restrict__ n_det, int max_det) {
    __shared__ float vwin[50][64];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    int wi[kScanMaxWakewords], mi[kScanMaxWakewords];
    BankLane r[kScanMaxWakewords];
    const int ref_len = load_ref_slots(rb, ref_rows + s * (size_t)ref_size, ref_size, cfg, wi, r);
    const int model_len = load_model_slots(mb, model_rows + s * (size_t)model_size, model_size, mi);
    const int max_len = table[s].max_len;
    const size_t rrow0 = s * (size_t)ref_size * (size_t)n_new, mrow0 = s * (size_t)model_size * (size_t)n_new;
    scan_live(
        vwin, lane, s, max_len, max_len > 0 && (ref_len > 0 || model_len > 0), vad_value, vad_mode_value, f0, n_new, cfg, state, out,
        [&](long long, int i) {
            Proposal p{false, 0.f, 0.f, -1, -1};
            propose_ref_slots(p, wi, r, ragg, ravg, rrow0, n_new, i);
            propose_model_slots(p, mi, magg, mavg, mlabel, mrow0, n_new, i);
            p.found = p.ww >= 0;
            return p;
        },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s, f, z, z.p_ww, z.p_label); });
}

hipError_t launch_scan_set_stream(hipStream_t st, const BankDev &b, const int32_t *stream_wakewords, int set_size, const float *agg,
                                  const float *avg, const float *vad_value, float vad_mode_value, size_t S, long long f0, int n_new,
                                  const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww, int32_t *det_label, int32_t *n_det,
                                  int max_det) {
    if (S == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_set_stream_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, b, stream_wakewords, set_size, agg, avg, vad_value,
                       vad_mode_value, S, f0, n_new, cfg, static_cast<StreamState *>(state), det, det_ww, det_label, n_det, max_det);
    return hipGetLastError();
}

hipError_t launch_scan_model_set_stream(hipStream_t st, const BankDev &b, const int32_t *stream_models, int set_size, const float *agg,
                                        const float *avg, const int32_t *label, const float *vad_value, float vad_mode_value, size_t S, long long f0,
                                        int n_new, const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww, int32_t *det_label,
                                        int32_t *n_det, int max_det) {
    if (S == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_model_set_stream_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, b, stream_models, set_size, agg, avg, label,
                       vad_value, vad_mode_value, S, f0, n_new, cfg, static_cast<StreamState *>(state), det, det_ww, det_label, n_det, max_det);
    return hipGetLastError();
}

hipError_t launch_scan_mixed_set_stream(hipStream_t st, const BankDev &rb, const int32_t *ref_rows, int ref_size, const BankDev &mb,
                                        const int32_t *model_rows, int model_size, const BankWakeword *table, const float *ragg, const float *ravg,
                                        const float *magg, const float *mavg, const int32_t *mlabel, const float *vad_value, float vad_mode_value,
                                        size_t S, long long f0, int n_new, const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww,
                                        int32_t *det_label, int32_t *n_det, int max_det) {
    if (S == 0) return hipSuccess;
    if (ref_size < 0 || ref_size > kScanMaxWakewords || model_size < 0 || model_size > kScanMaxWakewords || !table) return hipErrorInvalidValue;
    if ((ref_size && (!ref_rows || !ragg || !ravg)) || (model_size && (!model_rows || !magg || !mavg || !mlabel))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_mixed_set_stream_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, rb, ref_rows, ref_size, mb, model_rows, model_size,
                       table, ragg, ravg, magg, mavg, mlabel, vad_value, vad_mode_value, S, f0, n_new, cfg, static_cast<StreamState *>(state), det,
                       det_ww, det_label, n_det, max_det);
    return hipGetLastError();
}

}  // namespace rp
