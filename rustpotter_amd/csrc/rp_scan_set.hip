// rp_scan_set.hip -- the detection state machine (scan_frames, rp_scan.h) for streams that hold a SET of wakewords of a bank: a `Rustpotter`
// with several add_wakeword calls (src/detector.rs:304-346,433-447).  scan_set_kernel: whole recordings over the proposal rows of
// dtw_set_kernel; scan_set_stream_kernel: the new frames of a live call over the slot scores of dtw_set_stream_kernel, the state carried.
#include "rp_device.h"
#include "rp_scan.h"

namespace rp {

// (set_max_len, the window of a stream that holds a set, is in rp_scan.h: rp_scan_model_set.hip shares it)

// scan_bank_kernel for sets: the window length (and the countdown, Lmax(s) / 2) comes from the stream's set, the proposal of a window from
// the three rows dtw_set_kernel folded -- best_ww < 0: nobody proposes.  A stream without a live slot, or with fewer frames than its window,
// reports nothing.  A detection names the winner's BANK index.
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

hipError_t launch_scan_set(hipStream_t st, const BankDev &b, const int32_t *stream_wakewords, int set_size, const float *best, const float *best_avg,
                           const int32_t *best_ww, size_t win_pitch, const float *vad_value, float vad_mode_value, size_t S, size_t n_frames,
                           const ScanConfig &cfg, BatchDetection *det, int32_t *det_ww, int32_t *n_det, int max_det, uint32_t *hot) {
    if (S == 0) return hipSuccess;
    if (n_frames > 0x7fffffffULL || set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;   // a detection's frame is an int32
    hipLaunchKernelGGL(scan_set_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, b, stream_wakewords, set_size, best, best_avg, best_ww,
                       win_pitch, vad_value, vad_mode_value, S, n_frames, cfg, det, det_ww, n_det, max_det, hot);
    return hipGetLastError();
}

// scan_bank_stream_kernel for sets: agg / avg [S][set_size][n_new].  Per frame every live slot proposes with its own thresholds
// (bank_lane) and the best score wins, the first slot of equals: propose_best's rule (run_wakeword_detectors, src/detector.rs:433-447) with
// the bank index as the wakeword.  Window length, countdown and every threshold are read from the bank in this call.  A stream without a
// live slot reports nothing and keeps its state as it is (rp_stream_batch_set_wakeword_sets resets a stream it re-targets).
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
    const int32_t *set = stream_wakewords + s * (size_t)set_size;
    // the slots in registers: every loop over them is unrolled to the limit of a set
    int wi[kScanMaxWakewords];
    BankLane r[kScanMaxWakewords];
    int max_len = 0;
#pragma unroll
    for (int j = 0; j < kScanMaxWakewords; ++j) {
        wi[j] = j < set_size ? set[j] : -1;
        r[j] = bank_lane(b, wi[j], cfg);
        max_len = max(max_len, r[j].max_len);
    }
    int nd = 0;
    if (max_len > 0) {
        const size_t row0 = s * (size_t)set_size * (size_t)n_new;
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
                    const size_t row = row0 + (size_t)j * (size_t)n_new + i;
                    const float sj = agg[row];
                    float aj = 0.f;
                    bool pass = true;
                    if (r[j].avg_on) { aj = avg[row]; pass = !(aj < r[j].athr); }
                    if (pass && sj > r[j].thr && (p.ww < 0 || sj > p.score)) { p.ww = wi[j]; p.score = sj; p.avg = aj; }
                }
                p.found = p.ww >= 0;
                return p;
            },
            [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s, f, z, z.p_ww, -1); });
        stream_state_store(state + s, z, vwin, lane, vv != nullptr);
    }
    out.finish(s, nd);
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

}  // namespace rp
