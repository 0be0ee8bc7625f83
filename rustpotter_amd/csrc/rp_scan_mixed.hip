// rp_scan_mixed.hip -- the detection state machine (scan_frames, rp_scan.h) for streams that hold a MIXED set: wakeword references of a
// wakeword bank and models of a model bank on one detector, a `Rustpotter` with add_wakeword of both kinds (src/detector.rs:304-346,433-447).
// scan_mixed_set_kernel: whole recordings over the proposal rows of dtw_set_kernel and of nn_score_model_set_kernel;
// scan_mixed_set_stream_kernel: the new frames of a live call over the slot rows of dtw_mixed_stream_kernel and nn_score_set_stream_kernel, the
// state carried.  The fronts for sets of one kind are in rp_scan_set.hip and rp_scan_model_set.hip.
#include "rp_device.h"
#include "rp_scan.h"

namespace rp {

// scan_set_kernel / scan_model_set_kernel over both kinds.  The window of stream s is Lmax(s) frames, the longest over the live slots of both
// rows (table[s].max_len, mixed_targets_kernel), its countdown Lmax(s) / 2.  Either side's proposal rows were written for that side's own,
// shorter or equal, window: the window that starts at frame w is scored from frame w whatever Lmax is, so the rows are read as they are and
// only the windows f - Lmax(s) + 1 count.  Per window the better passing proposal wins, the reference of equals (references are added before
// models).  A side without a live slot for the stream is not read.  A detection names the winner's index in its own bank and, for a model,
// its label; -1 for a reference.
__global__ __launch_bounds__(64) void scan_mixed_set_kernel(MixedProposals refs, MixedProposals models, const BankWakeword *__restrict__ table,
                                                            size_t win_pitch, const float *__restrict__ vad_value, float vad_mode_value, size_t S,
                                                            size_t n_frames, ScanConfig cfg, BatchDetection *__restrict__ det,
                                                            int32_t *__restrict__ det_ww, int32_t *__restrict__ det_label,
                                                            int32_t *__restrict__ n_det, int max_det, uint32_t *__restrict__ hot) {
    __shared__ float vwin[50][64];  // VadDetector::window, one column per stream (lane)
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    bool candidate = true;
    if (hot) {
        candidate = hot[s] != 0u;
        if (candidate) hot[s] = 0u;   // consumed (Ctx::hot_flags)
    }
    const bool ref_live = refs.set_size > 0 && set_max_len(refs.bank, refs.rows + s * (size_t)refs.set_size, refs.set_size) > 0;
    const bool model_live = models.set_size > 0 && set_max_len(models.bank, models.rows + s * (size_t)models.set_size, models.set_size) > 0;
    const int max_len = table[s].max_len;
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    if (max_len == 0 || (!ref_live && !model_live) || !candidate || n_frames < (size_t)max_len) { out.finish(s, 0); return; }
    const size_t row0 = s * win_pitch;
    const float *vv = vad_value ? vad_value + s * n_frames : nullptr;
    if (vv)
        for (int i = 0; i < 50; ++i) vwin[i][lane] = __builtin_nanf("");
    ScanLane z = fresh_lane();
    const int nd = scan_frames(
        z, vwin, lane, vv, vad_mode_value, 0, (int)n_frames, max_len, cfg,
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
    out.finish(s, nd);
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

// scan_set_stream_kernel and scan_model_set_stream_kernel over both kinds, the state carried: the new frames of a live call over the
// reference slots' rows of dtw_mixed_stream_kernel (ragg / ravg [S][ref set][n_new]) and the model slots' rows of
// nn_score_set_stream_kernel (magg / mavg / mlabel [S][model set][n_new]).  Per frame every live reference slot proposes with its own
// thresholds (bank_lane, >), every live model slot where its score is not -2 (its gates were applied, >=); the best score wins, the first
// of equals in add_wakeword's order: reference slots, then model slots.  Window length and countdown are Lmax(s) of the table, prepared in
// this call.  The kind of a carried partial detection travels in p_label (-1: a reference; a passing model window always has a label), so
// a detection an earlier call's window won reports its kind, index and label.  A stream without a live slot reports nothing and keeps its
// state (rp_stream_batch_set_mixed_sets resets a stream it re-targets).
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
    // the slots in registers: every loop over them is unrolled to the limit of a set
    int wi[kScanMaxWakewords], mi[kScanMaxWakewords];
    BankLane r[kScanMaxWakewords];
    bool any_live = false;
#pragma unroll
    for (int j = 0; j < kScanMaxWakewords; ++j) {
        wi[j] = j < ref_size ? ref_rows[s * (size_t)ref_size + j] : -1;
        r[j] = bank_lane(rb, wi[j], cfg);
        mi[j] = j < model_size ? model_rows[s * (size_t)model_size + j] : -1;
        if (mi[j] < 0 || mi[j] >= mb.W) mi[j] = -1;
        any_live = any_live || !r[j].none || mi[j] >= 0;
    }
    const int max_len = table[s].max_len;
    int nd = 0;
    if (any_live && max_len > 0) {
        const size_t rrow0 = s * (size_t)ref_size * (size_t)n_new, mrow0 = s * (size_t)model_size * (size_t)n_new;
        const float *vv = vad_value ? vad_value + s * (size_t)n_new : nullptr;
        ScanLane z;
        stream_state_load(state + s, z, vwin, lane, vv != nullptr);
        nd = scan_frames(
            z, vwin, lane, vv, vad_mode_value, f0, n_new, max_len, cfg,
            [&](long long, int i) {
                Proposal p{false, 0.f, 0.f, -1, -1};
#pragma unroll
                for (int j = 0; j < kScanMaxWakewords; ++j) {
                    if (r[j].none) continue;
                    const size_t row = rrow0 + (size_t)j * (size_t)n_new + i;
                    const float sj = ragg[row];
                    float aj = 0.f;
                    bool pass = true;
                    if (r[j].avg_on) { aj = ravg[row]; pass = !(aj < r[j].athr); }
                    if (pass && sj > r[j].thr && (p.ww < 0 || sj > p.score)) { p.ww = wi[j]; p.score = sj; p.avg = aj; }
                }
#pragma unroll
                for (int j = 0; j < kScanMaxWakewords; ++j) {
                    if (mi[j] < 0) continue;
                    const size_t row = mrow0 + (size_t)j * (size_t)n_new + i;
                    const float sj = magg[row];
                    if (sj != -2.f && (p.ww < 0 || sj > p.score)) { p.ww = mi[j]; p.score = sj; p.avg = mavg[row]; p.label = mlabel[row]; }
                }
                p.found = p.ww >= 0;
                return p;
            },
            [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s, f, z, z.p_ww, z.p_label); });
        stream_state_store(state + s, z, vwin, lane, vv != nullptr);
    }
    out.finish(s, nd);
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
