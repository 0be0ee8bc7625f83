// rp_scan.hip -- the detection state machine over precomputed window scores (src/detector.rs:290-302,377-454, src/mfcc/vad.rs).
// scan_frames (rp_scan.h) is the state machine -- VAD gate, countdown, partial detection, reset after an emit -- and the only copy of it.  The
// four scan kernels here (and the two of rp_scan_sets.hip) run it, one lane per stream, and add what is their own: scan_kernel the whole
// recording of a detector with up to eight wakewords, scan_bank_kernel the same for a stream that holds one wakeword of a bank,
// scan_stream_kernel / scan_bank_stream_kernel the two over the new frames of a live call with the state carried between calls.  Also
// here: the VAD value kernels and the staging of live-stream batches.
#include "rp_device.h"
#include "rp_scan.h"

#include <cstddef>

namespace rp {

// ------------------------------------------------------------------------- VAD value
// mean(|mfcc|) of one frame, summed in coefficient order like VadDetector::is_voice (src/mfcc/vad.rs:12)
__device__ __forceinline__ float vad_value_of(const float *__restrict__ v, int K) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += fabsf(v[k]);
    return s / (float)K;
}

__global__ __launch_bounds__(256) void vad_value_kernel(const float *__restrict__ mfcc, size_t n, int K, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = vad_value_of(mfcc + i * K, K);
}

hipError_t launch_vad_value(hipStream_t st, const float *mfcc, size_t n_frames_total, int K, float *out) {
    if (n_frames_total == 0) return hipSuccess;
    const size_t blocks = (n_frames_total + 255) / 256;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vad_value_kernel, dim3((unsigned)blocks), dim3(256), 0, st, mfcc, n_frames_total, K, out);
    return hipGetLastError();
}

// the same over rows of `pitch` frames: out [S][n] from mfcc [S][pitch][K]
__global__ __launch_bounds__(256) void vad_value_rows_kernel(const float *__restrict__ mfcc, size_t S, size_t n, size_t pitch, int K,
                                                             float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= S * n) return;
    const size_t s = i / n, f = i - s * n;
    out[i] = vad_value_of(mfcc + (s * pitch + f) * K, K);
}
hipError_t launch_vad_value_rows(hipStream_t st, const float *mfcc, size_t S, size_t n, size_t pitch, int K, float *out) {
    if (S * n == 0) return hipSuccess;
    const size_t blocks = (S * n + 255) / 256;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vad_value_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, mfcc, S, n, pitch, K, out);
    return hipGetLastError();
}

// run_wakeword_detectors, src/detector.rs:433-447: every wakeword whose own thresholds pass proposes a detection, the best score wins
// (the first of equals).  `row` is the window's element of every wakeword's agg / avg / label.
__device__ __forceinline__ Proposal propose_best(const ScanWakewords &ww, size_t row) {
    Proposal p{false, 0.f, 0.f, -1, -1};
    for (int j = 0; j < ww.n; ++j) {
        const float sj = ww.agg[j][row];
        float aj = 0.f;
        bool pass = true;
        if (ww.avg[j]) { aj = ww.avg[j][row]; pass = !(aj < ww.avg_threshold[j]); }
        if (pass && sj > ww.threshold[j] && (p.ww < 0 || sj > p.score)) { p.ww = j; p.score = sj; p.avg = aj; }
    }
    p.found = p.ww >= 0;
    if (p.found && ww.label[p.ww]) p.label = ww.label[p.ww][row];
    return p;
}
// the one wakeword wi of such a stream: `row` is the window's element of the stream's agg / avg
__device__ __forceinline__ Proposal propose_one(const float *__restrict__ agg, const float *__restrict__ avg, size_t row, float thr, float athr,
                                                bool avg_on, int wi) {
    Proposal p{false, agg[row], 0.f, wi, -1};
    bool pass = true;
    if (avg_on) { p.avg = avg[row]; pass = !(p.avg < athr); }
    p.found = pass && p.score > thr;
    return p;
}

// ------------------------------------------------------------------------- whole recordings
// One detector with ww.n wakewords of one window length over S recordings of n_frames frames; the window ending at frame f is element
// f - max_len + 1 of the stream's row of n_win scores.  Its own: the front that finds the streams with a window that can fire.  det_ww
// gets the window's label where the winning wakeword is a model, else the wakeword's index.
__global__ __launch_bounds__(64) void scan_kernel(ScanWakewords ww, const float *__restrict__ vad_value, float vad_mode_value,
                                                  size_t S, size_t n_frames, ScanConfig cfg, BatchDetection *__restrict__ det,
                                                  int32_t *__restrict__ det_ww, int32_t *__restrict__ n_det, int max_det) {
    __shared__ float vwin[50][64];  // VadDetector::window, one column per stream (lane)
    __shared__ unsigned long long candidates;  // bit r: stream r of this block has a window that can fire
    const int lane = threadIdx.x;
    const long max_len = cfg.max_len;
    const long n_win = (long)n_frames - max_len + 1;
    // A detection needs at least one window whose aggregate passes the thresholds (run_detection :411-429;
    // the VAD only gates).  The wave first sweeps the block's 64 score rows with coalesced loads; streams
    // without such a window (all of them on non-matching audio) are done, the others run the state machine.
    // When the aggregate pass has already raised a flag per stream (ww.hot), that flag is the answer and nothing is swept.
    bool candidate = true;
    if (ww.hot) {
        const size_t sh = (size_t)blockIdx.x * 64 + lane;
        candidate = sh < S && ww.hot[sh] != 0u;
        if (candidate) ww.hot[sh] = 0u;   // consumed: the flags are zero again for the context's next call (no memset per call; Ctx::hot_flags)
    } else {
        if (lane == 0) candidates = 0;
        __syncthreads();
        const size_t s0 = (size_t)blockIdx.x * 64;
        const size_t rows = S - s0 < 64 ? S - s0 : 64;
        const size_t total = n_win > 0 ? rows * (size_t)n_win : 0;  // the block's score rows are one contiguous range
        unsigned long long mask = 0;
        for (int j = 0; j < ww.n; ++j) {
            const float *a0 = ww.agg[j] + s0 * (size_t)(n_win > 0 ? n_win : 0);
            const float *v0 = ww.avg[j] ? ww.avg[j] + s0 * (size_t)(n_win > 0 ? n_win : 0) : nullptr;
            // eight rows' loads in flight per wait (one load -> wait -> test per element made a block's 64 x n_win aggregates n_win
            // dependent round trips: 0.17 ms for 4 096 streams x 202 windows in the batched model detector)
            const float thr = ww.threshold[j], athr = ww.avg_threshold[j];
            if (v0) {
#pragma unroll 8
                for (size_t e = lane; e < total; e += 64) {
                    const float a = a0[e], v = v0[e];
                    if (a > thr && !(v < athr)) mask |= 1ull << (e / (size_t)n_win);
                }
            } else {
#pragma unroll 8
                for (size_t e = lane; e < total; e += 64)
                    if (a0[e] > thr) mask |= 1ull << (e / (size_t)n_win);
            }
        }
        if (mask) atomicOr(&candidates, mask);
        __syncthreads();
        candidate = (candidates >> lane) & 1ull;
    }
    size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const ScanOut out{det, det_ww, nullptr, n_det, max_det};
    if (!candidate) { out.finish(s, 0); return; }
    const size_t row0 = s * (size_t)(n_win > 0 ? n_win : 0);
    const float *vv = vad_value ? vad_value + s * n_frames : nullptr;
    if (vv)
        for (int i = 0; i < 50; ++i) vwin[i][lane] = __builtin_nanf("");
    ScanLane z = fresh_lane();
    const int nd = scan_frames(
        z, vwin, lane, vv, vad_mode_value, 0, (int)n_frames, cfg.max_len, cfg,
        [&](long long f, int) { return propose_best(ww, row0 + (size_t)(f - max_len + 1)); },
        [&](int nd, long long f, const ScanLane &z) {
            out.put(s, nd, (int32_t)s + cfg.stream_base, f, z, ww.label[z.p_ww] ? z.p_label : z.p_ww, -1);
        });
    out.finish(s, nd);
}

hipError_t launch_scan_multi(hipStream_t st, const ScanWakewords &ww, const float *vad_value, float vad_mode_value, size_t S,
                             size_t n_frames, const ScanConfig &cfg, BatchDetection *det, int32_t *det_ww, int32_t *n_det, int max_det) {
    if (S == 0) return hipSuccess;
    if (ww.n < 1 || ww.n > kScanMaxWakewords || n_frames > 0x7fffffffULL) return hipErrorInvalidValue;   // a detection's frame is an int32
    size_t blocks = (S + 63) / 64;
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)blocks), dim3(64), 0, st, ww, vad_value, vad_mode_value, S, n_frames, cfg, det, det_ww,
                       n_det, max_det);
    return hipGetLastError();
}

hipError_t launch_scan(hipStream_t st, const float *agg, const float *avg, const float *vad_value, float vad_mode_value,
                       size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det, int32_t *n_det, int max_det,
                       uint32_t *hot) {
    ScanWakewords ww{};
    ww.n = 1;
    ww.hot = hot;
    ww.agg[0] = agg; ww.avg[0] = cfg.avg_enabled ? avg : nullptr;
    ww.threshold[0] = cfg.threshold; ww.avg_threshold[0] = cfg.avg_threshold;
    return launch_scan_multi(st, ww, vad_value, vad_mode_value, S, n_frames, cfg, det, nullptr, n_det, max_det);
}

// The same for a wakeword bank (rp_dtw_bank.hip): stream s holds the one wakeword bank[stream_wakeword[s]] (bank_lane), so the window
// length is a per-lane value; its rows are agg / avg + s * win_pitch.  A stream without a wakeword, or with fewer frames than its
// window, reports nothing.  `hot` as in scan_kernel: the flags dtw_bank_kernel raised, put back to 0 here.
__global__ __launch_bounds__(64) void scan_bank_kernel(BankDev b, const int32_t *__restrict__ stream_wakeword, const float *__restrict__ agg,
                                                       const float *__restrict__ avg, size_t win_pitch, const float *__restrict__ vad_value,
                                                       float vad_mode_value, size_t S, size_t n_frames, ScanConfig cfg,
                                                       BatchDetection *__restrict__ det, int32_t *__restrict__ n_det, int max_det,
                                                       uint32_t *__restrict__ hot) {
    __shared__ float vwin[50][64];  // VadDetector::window, one column per stream (lane)
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const int wi = stream_wakeword[s];
    const BankLane r = bank_lane(b, wi, cfg);
    const int max_len = r.max_len;
    const ScanOut out{det, nullptr, nullptr, n_det, max_det};
    const bool avg_on = avg && r.avg_on;
    const size_t row0 = s * win_pitch;
    scan_recording(
        vwin, lane, s, hot, max_len, !r.none, vad_value, vad_mode_value, n_frames, cfg, out,
        [&](long long f, int) { return propose_one(agg, avg, row0 + (size_t)(f - max_len + 1), r.thr, r.athr, avg_on, wi); },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s + cfg.stream_base, f, z, 0, -1); });
}

hipError_t launch_scan_bank(hipStream_t st, const BankDev &b, const int32_t *stream_wakeword, const float *agg, const float *avg, size_t win_pitch,
                            const float *vad_value, float vad_mode_value, size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det,
                            int32_t *n_det, int max_det, uint32_t *hot) {
    if (S == 0) return hipSuccess;
    if (n_frames > 0x7fffffffULL) return hipErrorInvalidValue;   // a detection's frame is an int32
    hipLaunchKernelGGL(scan_bank_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, b, stream_wakeword, agg, avg, win_pitch, vad_value,
                       vad_mode_value, S, n_frames, cfg, det, n_det, max_det, hot);
    return hipGetLastError();
}

// ------------------------------------------------------------- streaming batches
// hist [S][hist_pitch] = the last 480-sample chunk of the previous call (old_hist row + old_off) | the new chunks decoded
template <class TIN>
__global__ __launch_bounds__(256) void stream_stage_kernel(const TIN *__restrict__ pcm, int channels, size_t S, size_t n_new,
                                                           size_t pcm_stride, const float *__restrict__ old_hist, size_t old_off,
                                                           float *__restrict__ hist, size_t hist_pitch) {
    const size_t row = kFrame + n_new, total = S * row;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t s = i / row, k = i - s * row;
        hist[s * hist_pitch + k] = k < (size_t)kFrame ? old_hist[s * hist_pitch + old_off + k]
                                                      : SampleIn<TIN>::cvt(pcm[s * pcm_stride + (k - kFrame) * channels]);
    }
}
// rows [S][src_pitch] -> [S][dst_pitch]: dst[s][0..count) = src[s][src_off .. src_off+count)
__global__ __launch_bounds__(256) void carry_rows_kernel(const float *src, size_t S, size_t src_pitch, size_t src_off, size_t count,
                                                         float *dst, size_t dst_pitch) {
    const size_t total = S * count;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t s = i / count, k = i - s * count;
        dst[s * dst_pitch + k] = src[s * src_pitch + src_off + k];
    }
}

hipError_t launch_stream_stage(hipStream_t st, const void *pcm, int fmt, int channels, size_t S, size_t n_new, size_t pcm_stride,
                               const float *old_hist, size_t old_off, float *hist, size_t hist_pitch) {
    if (S == 0 || n_new == 0) return hipSuccess;
    size_t blocks = (S * (kFrame + n_new) + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    switch (fmt) {
    case 0: hipLaunchKernelGGL(stream_stage_kernel<int8_t>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const int8_t *>(pcm), channels, S, n_new, pcm_stride, old_hist, old_off, hist, hist_pitch); break;
    case 1: hipLaunchKernelGGL(stream_stage_kernel<int16_t>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const int16_t *>(pcm), channels, S, n_new, pcm_stride, old_hist, old_off, hist, hist_pitch); break;
    case 2: hipLaunchKernelGGL(stream_stage_kernel<int32_t>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const int32_t *>(pcm), channels, S, n_new, pcm_stride, old_hist, old_off, hist, hist_pitch); break;
    case 3: hipLaunchKernelGGL(stream_stage_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const float *>(pcm), channels, S, n_new, pcm_stride, old_hist, old_off, hist, hist_pitch); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_carry_rows(hipStream_t st, const float *src, size_t S, size_t src_pitch, size_t src_off, size_t count, float *dst,
                             size_t dst_pitch) {
    if (S == 0 || count == 0) return hipSuccess;
    size_t blocks = (S * count + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(carry_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, S, src_pitch, src_off, count, dst, dst_pitch);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void stream_state_init_kernel(StreamState *__restrict__ st, size_t S) {
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    StreamState z;
    z.lane = fresh_lane();
    for (int i = 0; i < 50; ++i) z.vad_window[i] = __builtin_nanf("");
    st[s] = z;
}
hipError_t launch_stream_state_init(hipStream_t st, void *state, size_t S) {
    if (S == 0) return hipSuccess;
    hipLaunchKernelGGL(stream_state_init_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, static_cast<StreamState *>(state), S);
    return hipGetLastError();
}
size_t stream_state_bytes() { return sizeof(StreamState); }

// Rustpotter::reset (src/detector.rs:290-302) for one stream (or all, stream < 0): the next chunk only refills
// the extractor, so the next frame seen is `resume`.
__global__ __launch_bounds__(64) void stream_state_reset_kernel(StreamState *__restrict__ st, size_t first, size_t n, long long resume) {
    const size_t s = first + (size_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= first + n) return;
    StreamState z = st[s];
    lane_reset(z.lane, resume);
    for (int i = 0; i < 50; ++i) z.vad_window[i] = __builtin_nanf("");
    st[s] = z;
}
hipError_t launch_stream_state_reset_range(hipStream_t st, void *state, size_t S, size_t first, size_t n, long long resume) {
    if (n == 0) return hipSuccess;
    if (first > S || n > S - first) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_state_reset_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, static_cast<StreamState *>(state), first, n,
                       resume);
    return hipGetLastError();
}
hipError_t launch_stream_state_reset(hipStream_t st, void *state, size_t S, long long stream, long long resume) {
    if (stream >= 0 && (size_t)stream >= S) return hipSuccess;   // no such stream: nothing to reset, as before
    return stream < 0 ? launch_stream_state_reset_range(st, state, S, 0, S, resume)
                      : launch_stream_state_reset_range(st, state, S, (size_t)stream, 1, resume);
}

// scan_kernel's detector (several wakewords, run_wakeword_detectors) on live streams: det_ww gets the winning wakeword's index,
// det_label the window's label where that wakeword is a model, else -1.
__global__ __launch_bounds__(64) void scan_stream_kernel(ScanWakewords ww, const float *__restrict__ vad_value, float vad_mode_value, size_t S,
                                                         long long f0, int n_new, ScanConfig cfg, StreamState *__restrict__ state,
                                                         BatchDetection *__restrict__ det, int32_t *__restrict__ det_ww,
                                                         int32_t *__restrict__ det_label, int32_t *__restrict__ n_det, int max_det) {
    __shared__ float vwin[50][64];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    const size_t row0 = s * (size_t)n_new;
    scan_live(
        vwin, lane, s, cfg.max_len, true, vad_value, vad_mode_value, f0, n_new, cfg, state, out,
        [&](long long, int i) { return propose_best(ww, row0 + i); },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s, f, z, z.p_ww, z.p_label); });
}

hipError_t launch_scan_stream_multi(hipStream_t st, const ScanWakewords &ww, const float *vad_value, float vad_mode_value, size_t S,
                                    long long f0, int n_new, const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww,
                                    int32_t *det_label, int32_t *n_det, int max_det) {
    if (S == 0) return hipSuccess;
    if (ww.n < 1 || ww.n > kScanMaxWakewords) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_stream_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, ww, vad_value, vad_mode_value, S, f0, n_new, cfg,
                       static_cast<StreamState *>(state), det, det_ww, det_label, n_det, max_det);
    return hipGetLastError();
}

// scan_bank_kernel's detector on live streams (rp_stream_batch_new_bank): stream s holds the one wakeword bank[stream_wakeword[s]]
// (bank_lane); agg / avg [S][n_new].  A detection reports the stream's bank index as its wakeword and label -1.  A stream without a
// wakeword reports nothing and keeps its state as it is (rp_stream_batch_set_wakewords resets a stream it re-targets).
// label (optional, [S][n_new]; a batch over a model bank, b = ModelBank::scan): the label of every window; the proposing window's travels in
// the stream's state (p_label, as in scan_stream_kernel), so a detection reports the label of its best window even when an earlier call
// scored it.
__global__ __launch_bounds__(64) void scan_bank_stream_kernel(BankDev b, const int32_t *__restrict__ stream_wakeword, const float *__restrict__ agg,
                                                              const float *__restrict__ avg, const float *__restrict__ vad_value,
                                                              float vad_mode_value, size_t S, long long f0, int n_new, ScanConfig cfg,
                                                              StreamState *__restrict__ state, BatchDetection *__restrict__ det,
                                                              int32_t *__restrict__ det_ww, int32_t *__restrict__ det_label,
                                                              int32_t *__restrict__ n_det, int max_det, const int32_t *__restrict__ label) {
    __shared__ float vwin[50][64];
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * 64 + lane;
    if (s >= S) return;
    const ScanOut out{det, det_ww, det_label, n_det, max_det};
    const int wi = stream_wakeword[s];
    const BankLane r = bank_lane(b, wi, cfg);
    const size_t row0 = s * (size_t)n_new;
    scan_live(
        vwin, lane, s, r.max_len, !r.none, vad_value, vad_mode_value, f0, n_new, cfg, state, out,
        [&](long long, int i) {
            Proposal p = propose_one(agg, avg, row0 + i, r.thr, r.athr, r.avg_on, wi);
            if (label) p.label = label[row0 + i];
            return p;
        },
        [&](int nd, long long f, const ScanLane &z) { out.put(s, nd, (int32_t)s, f, z, z.p_ww, label ? z.p_label : -1); });
}

hipError_t launch_scan_bank_stream(hipStream_t st, const BankDev &b, const int32_t *stream_wakeword, const float *agg, const float *avg,
                                   const float *vad_value, float vad_mode_value, size_t S, long long f0, int n_new, const ScanConfig &cfg,
                                   void *state, BatchDetection *det, int32_t *det_ww, int32_t *det_label, int32_t *n_det, int max_det,
                                   const int32_t *label) {
    if (S == 0) return hipSuccess;
    hipLaunchKernelGGL(scan_bank_stream_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, b, stream_wakeword, agg, avg, vad_value,
                       vad_mode_value, S, f0, n_new, cfg, static_cast<StreamState *>(state), det, det_ww, det_label, n_det, max_det, label);
    return hipGetLastError();
}

}  // namespace rp
