// rp_mlp_model_set.hip -- MODEL SETS: stream s holds up to kScanMaxWakewords models of a model bank, sets [S][set_size] (outside [0, W): an
// empty slot) -- a `Rustpotter` with several add_wakeword calls of wakeword models (src/detector.rs:304-346,433-447, wakeword_nn.rs:137).
// The detector's window is Lmax(s) frames, the longest train_size of the stream's live slots; slot j scores the OLDEST L_j frames of it.
// Here: the window means, the two forwards (whole recordings, live) and the decision kernels; the scan fronts are in rp_scan_sets.hip, the
// calls in rp_bank_calls.cpp and rp_stream_batch.cpp.  DESIGN.md §4.4.
//
// WHOLE RECORDINGS (mlp_windows_model_set_kernel<NT>, 1 .. 7 tiles; 256 threads, two workgroups per CU as mlp_windows_bank_kernel): a front
// of mlp_windows_body (rp_mlp_windows.h) over rows (s, j).  The window count and the cut into workgroups come from the SET, n_win_s =
// n_frames - Lmax(s) + 1, the window means and the model from slot j -- so row (s, j) has the bits of rp_mlp_forward_windows_bank over the
// first n_frames - (Lmax(s) - L_j) frames of the stream with that model alone.  An empty slot, and every slot of a stream shorter than
// Lmax(s), reads no image and keeps the zero rows the launcher wrote.
//
// LIVE (mlp_set_stream_kernel<RT>, RT = 1 or 2 tiles of 16 rows a wave; 64 threads; built for three and two waves per SIMD, at most 168 and
// 256 registers, no spills, no scratch -- the occupancy of mlp_bank_stream_kernel<RT>, whose body it shares, rp_mlp_bank_stream.h): one
// wave per (s, j, row tile).  The first window of the call starts Lmax(s) - 1 frames before the first new frame for EVERY slot; slot j reads
// L_j frames from there.  Row by row the arithmetic of mlp_mfma_kernel<.., kMlpBf16x3> in window mode.
//
// COST MODEL (tools/bench_model_bank_sets.py measures; DESIGN.md §4.4 has the figures): the forward reads one layer-1 image per live slot, as set_size
// model-bank calls would; what a set saves is the front end, the MFCC and the scan.
#include "rp_mlp_bank_stream.h"
#include "rp_mlp_windows.h"
#include "rp_host.h"

namespace rp {

// on_wakeword_change, src/detector.rs:328-334: the window of a detector is as long as its longest wakeword; 0: no live slot
__device__ __forceinline__ int model_set_max_len(const ModelBankDev &b, const int32_t *__restrict__ set, int set_size) {
    int lmax = 0;
    for (int j = 0; j < set_size; ++j) {
        const int mi = set[j];
        if (mi >= 0 && mi < b.W) lmax = max(lmax, b.e[mi].L);
    }
    return lmax;
}

// ------------------------------------------------------------------------------------------------------------------ whole recordings
// window means of rows (s, j): the windows start where the set's do and are L_j frames long; mean [S][set_size][win_pitch][16]
__global__ __launch_bounds__(256) void window_means_model_set_kernel(ModelBankDev b, const int32_t *__restrict__ sets, int set_size,
                                                                     const float *__restrict__ mfcc, size_t n_frames, unsigned tiles,
                                                                     size_t win_pitch, float *__restrict__ mean) {
    const size_t row = blockIdx.x / tiles;
    const size_t w0 = (size_t)(blockIdx.x - row * tiles) * 64;
    const size_t s = row / (size_t)set_size;
    const int mi = sets[row];
    if (mi < 0 || mi >= b.W) return;
    const int lmax = model_set_max_len(b, sets + s * (size_t)set_size, set_size);
    if (n_frames < (size_t)lmax) return;
    const size_t n_win = n_frames - (size_t)lmax + 1;
    if (w0 >= n_win) return;
    const size_t nw = n_win - w0 < 64 ? n_win - w0 : 64;
    window_means_body(mfcc + (s * n_frames + w0) * 16, (int)nw, b.e[mi].L, 16, mean + (row * win_pitch + w0) * 16);
}

template <int NT>
__global__ __launch_bounds__(64 * kWinWaves, 2) void mlp_windows_model_set_kernel(ModelBankDev bank, const int32_t *__restrict__ sets, int set_size,
                                                                                  const float *__restrict__ mfcc, size_t n_frames, unsigned grid_bps,
                                                                                  const float *__restrict__ mean, size_t win_pitch,
                                                                                  float *__restrict__ out) {
    const size_t row = blockIdx.x / grid_bps;   // (s, j)
    const unsigned b = blockIdx.x - (unsigned)row * grid_bps;
    const size_t s = row / (size_t)set_size;
    const int mi = sets[row];
    if (mi < 0 || mi >= bank.W) return;   // an empty slot: the row stays zero
    const int lmax = model_set_max_len(bank, sets + s * (size_t)set_size, set_size);
    if (n_frames < (size_t)lmax) return;
    const ModelBankEntry e = bank.e[mi];
    const size_t n_win = n_frames - (size_t)lmax + 1;   // the set's count, not the model's own
    const WinCut cut = mlp_windows_cut(n_win);
    if (b >= cut.bps || cut.tiles > NT) return;
    const size_t w0 = (size_t)b * (size_t)(cut.tiles * kWinTile);
    const WinModel m{e.L, static_cast<const u32x4 *>(bank.wimg) + e.wimg, e.n1p, bank.b1 + e.b1, bank.wsum + e.wsum, bank.tail + e.tail,
                     e.tail_floats, e.n_layers, e.d1, e.d2, e.d3};
    const WinWork k{mfcc + (s * n_frames + w0) * 16, mean + row * win_pitch * 16, out + row * win_pitch * (size_t)bank.label_pitch,
                    (size_t)bank.label_pitch, w0, n_win, mlp_windows_slots(cut.tiles, e.L), cut.tiles, nullptr, 0, 0};
    mlp_windows_body<NT, true>(m, k);
}

void model_set_shape_add(ModelBankShape *sh, size_t n_frames, int lmax, int L, int tail_floats) {
    if (L < 1 || lmax < L || n_frames < (size_t)lmax) return;
    const WinCut cut = mlp_windows_cut(n_frames - (size_t)lmax + 1);
    sh->nt = std::max(sh->nt, cut.tiles);
    sh->bps = std::max(sh->bps, cut.bps);
    sh->lds = std::max(sh->lds, mlp_windows_lds(tail_floats, mlp_windows_slots(cut.tiles, L), kWinMaxTiles, 3, 0));
}

hipError_t launch_window_means_model_set(hipStream_t st, const ModelBankDev &b, const int32_t *sets, int set_size, const float *mfcc, size_t S,
                                         size_t n_frames, size_t win_pitch, float *mean) {
    if (S == 0 || win_pitch == 0 || b.W == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    const size_t tiles = (win_pitch + 63) / 64, blocks = tiles * S * (size_t)set_size;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = (size_t)(64 + 256 - 1) * 16 * sizeof(float);   // the bank's longest window: 256 frames
    hipLaunchKernelGGL(window_means_model_set_kernel, dim3((unsigned)blocks), dim3(256), lds, st, b, sets, set_size, mfcc, n_frames, (unsigned)tiles,
                       win_pitch, mean);
    return hipGetLastError();
}

hipError_t launch_mlp_windows_model_set(hipStream_t st, const ModelBankDev &b, const ModelBankShape &sh, const int32_t *sets, int set_size,
                                        const float *mfcc, size_t S, size_t n_frames, const float *mean, size_t win_pitch, float *logits) {
    if (S == 0 || win_pitch == 0 || b.label_pitch == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    const size_t rows = S * (size_t)set_size;
    if (hipError_t e = hipMemsetAsync(logits, 0, rows * win_pitch * (size_t)b.label_pitch * sizeof(float), st); e != hipSuccess) return e;
    if (sh.nt == 0 || sh.bps == 0) return hipSuccess;   // no stream of the call has a window
    if (rows * sh.bps > 0x7fffffffULL || sh.lds > 160 * 1024) return hipErrorInvalidValue;
    return mlp_windows_tiles(sh.nt, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(mlp_windows_model_set_kernel<NT>), 160 * 1024); e != hipSuccess) return e;
        hipLaunchKernelGGL(mlp_windows_model_set_kernel<NT>, dim3((unsigned)(rows * sh.bps)), dim3(64 * kWinWaves), sh.lds, st, b, sets, set_size, mfcc,
                           n_frames, sh.bps, mean, win_pitch, logits);
        return hipGetLastError();
    });
}

// The decision of every window of every stream: each live slot's label, score and average score as nn_score_bank_kernel computes them, then
// run_wakeword_detectors' rule (src/detector.rs:433-447): the best passing score wins, the first slot of equals.  Rows [S][win_pitch]: best
// (-2: nobody proposes), its average score, the winner's BANK index (-1) and its label (-1).
__global__ __launch_bounds__(256) void nn_score_model_set_kernel(ModelBankDev b, const int32_t *__restrict__ sets, int set_size,
                                                                 const float *__restrict__ logits, size_t S, size_t n_frames, size_t win_pitch,
                                                                 float ref, int calc_avg, float threshold, float avg_threshold,
                                                                 float *__restrict__ best, float *__restrict__ best_avg, int32_t *__restrict__ best_ww,
                                                                 int32_t *__restrict__ best_label, uint32_t *__restrict__ hot) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= S * win_pitch) return;
    const size_t s = r / win_pitch, w = r - s * win_pitch;
    const int32_t *set = sets + s * (size_t)set_size;
    const int lmax = model_set_max_len(b, set, set_size);
    float bs = -2.f, ba = 0.f;
    int bw = -1, bl = -1;
    if (lmax > 0 && n_frames >= (size_t)lmax && w < n_frames - (size_t)lmax + 1) {
        for (int j = 0; j < set_size; ++j) {
            const int mi = set[j];
            if (mi < 0 || mi >= b.W) continue;
            const ModelBankEntry e = b.e[mi];
            float score, av;
            int li;
            nn_score_row(logits + ((s * (size_t)set_size + j) * win_pitch + w) * (size_t)b.label_pitch, e.n_labels, e.none_index, ref, calc_avg, threshold,
                         avg_threshold, &score, &av, &li);
            if (score != -2.f && (bw < 0 || score > bs)) { bs = score; ba = av; bw = mi; bl = li; }
        }
    }
    best[r] = bs; best_avg[r] = ba; best_ww[r] = bw; best_label[r] = bl;
    if (hot && bw >= 0) hot[s] = 1u;   // (every writer stores the same value)
}

hipError_t launch_nn_score_model_set(hipStream_t st, const ModelBankDev &b, const int32_t *sets, int set_size, const float *logits, size_t S,
                                     size_t n_frames, size_t win_pitch, float score_ref10, int calc_avg, float threshold, float avg_threshold,
                                     float *best, float *best_avg, int32_t *best_ww, int32_t *best_label, uint32_t *hot) {
    const size_t blocks = (S * win_pitch + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffULL || set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_score_model_set_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b, sets, set_size, logits, S, n_frames, win_pitch,
                       score_ref10, calc_avg, threshold, avg_threshold, best, best_avg, best_ww, best_label, hot);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ live
// window means of rows (s, j) of a live call: new window i of the stream starts at frame fill - (Lmax(s) - 1) + i, slot j's is L_j frames
// long; mean [S][set_size][n_new][16].  Rows of empty slots are not written (nobody reads them).
__global__ __launch_bounds__(256) void window_means_set_stream_kernel(ModelBankDev b, const int32_t *__restrict__ sets, int set_size,
                                                                      const float *__restrict__ frames, size_t cap, size_t fill, size_t n_new,
                                                                      unsigned tiles, float *__restrict__ mean) {
    const size_t row = blockIdx.x / tiles;
    const size_t w0 = (size_t)(blockIdx.x - row * tiles) * 64;
    const size_t s = row / (size_t)set_size;
    const int mi = sets[row];
    if (mi < 0 || mi >= b.W) return;
    const int lmax = model_set_max_len(b, sets + s * (size_t)set_size, set_size);
    const size_t nw = n_new - w0 < 64 ? n_new - w0 : 64;
    window_means_body(frames + (s * cap + fill - (size_t)(lmax - 1) + w0) * 16, (int)nw, b.e[mi].L, 16, mean + (row * n_new + w0) * 16);
}

template <int RT>
__global__ __launch_bounds__(64, RT == 1 ? 3 : 2) void mlp_set_stream_kernel(ModelBankDev bank, const int32_t *__restrict__ sets, int set_size,
                                                                             const float *__restrict__ frames, size_t cap, size_t fill, int n_new,
                                                                             unsigned wps, const float *__restrict__ mean, float *__restrict__ out) {
    __shared__ float h1[16 * kBsH1], h2[16 * kBsH1];
    const size_t row = blockIdx.x / wps;   // (s, j)
    const int r0 = (int)(blockIdx.x - (unsigned)row * wps) * (16 * RT);   // first new window of this wave
    const size_t s = row / (size_t)set_size;
    const int label_pitch = bank.label_pitch;
    float *out_s = out + row * (size_t)n_new * (size_t)label_pitch;
    const int mi = sets[row];
    if (mi < 0 || mi >= bank.W) {   // an empty slot: zero rows
        const int rows_here = n_new - r0 < 16 * RT ? n_new - r0 : 16 * RT;
        for (int i = threadIdx.x; i < rows_here * label_pitch; i += 64) out_s[(size_t)r0 * (size_t)label_pitch + i] = 0.f;
        return;
    }
    const int lmax = model_set_max_len(bank, sets + s * (size_t)set_size, set_size);
    const ModelBankEntry e = bank.e[mi];
    mlp_bank_stream_body<RT>(bank, e, frames + (s * cap + fill - (size_t)(lmax - 1)) * 16, mean + row * (size_t)n_new * 16, out_s, n_new, r0, h1, h2);
}

hipError_t launch_window_means_set_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *sets, int set_size, const float *frames,
                                          size_t S, size_t cap, size_t fill, size_t n_new, float *mean) {
    if (S == 0 || n_new == 0 || b.W == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    if (max_L < 1 || max_L > 256 || fill + 1 < (size_t)max_L || fill + n_new > cap) return hipErrorInvalidValue;   // every window lies inside its row
    const size_t tiles = (n_new + 63) / 64, blocks = tiles * S * (size_t)set_size;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = ((n_new < 64 ? n_new : 64) + (size_t)max_L - 1) * 16 * sizeof(float);
    hipLaunchKernelGGL(window_means_set_stream_kernel, dim3((unsigned)blocks), dim3(256), lds, st, b, sets, set_size, frames, cap, fill, n_new,
                       (unsigned)tiles, mean);
    return hipGetLastError();
}

hipError_t launch_mlp_set_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *sets, int set_size, const float *frames, size_t S,
                                 size_t cap, size_t fill, size_t n_new, const float *mean, float *logits) {
    if (S == 0 || n_new == 0 || b.W == 0 || b.label_pitch == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    if (max_L < 1 || fill + 1 < (size_t)max_L || fill + n_new > cap || n_new > 0x7fffffffULL) return hipErrorInvalidValue;
    const int rt = n_new > 16 ? 2 : 1;
    const size_t wps = (n_new + 16 * rt - 1) / (16 * rt), blocks = S * (size_t)set_size * wps;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    if (rt == 1)
        hipLaunchKernelGGL(mlp_set_stream_kernel<1>, dim3((unsigned)blocks), dim3(64), 0, st, b, sets, set_size, frames, cap, fill, (int)n_new,
                           (unsigned)wps, mean, logits);
    else
        hipLaunchKernelGGL(mlp_set_stream_kernel<2>, dim3((unsigned)blocks), dim3(64), 0, st, b, sets, set_size, frames, cap, fill, (int)n_new,
                           (unsigned)wps, mean, logits);
    return hipGetLastError();
}

// nn_score_bank_stream_kernel over the slot rows [S][set_size][n_new]: every live slot's score (-2: no valid detection), average score and
// label; an empty slot: -2, 0, -1.  The scan (scan_model_set_stream_kernel) picks the winner of a window.
__global__ __launch_bounds__(256) void nn_score_set_stream_kernel(ModelBankDev b, const int32_t *__restrict__ sets, const float *__restrict__ logits,
                                                                  size_t rows, size_t n_new, float ref, int calc_avg, float threshold,
                                                                  float avg_threshold, float *__restrict__ agg, float *__restrict__ avg,
                                                                  int32_t *__restrict__ label) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows * n_new) return;
    const int mi = sets[r / n_new];
    float score = -2.f, av = 0.f;
    int bi = -1;
    if (mi >= 0 && mi < b.W) {
        const ModelBankEntry e = b.e[mi];
        nn_score_row(logits + r * (size_t)b.label_pitch, e.n_labels, e.none_index, ref, calc_avg, threshold, avg_threshold, &score, &av, &bi);
    }
    agg[r] = score; avg[r] = av; label[r] = bi;
}

hipError_t launch_nn_score_set_stream(hipStream_t st, const ModelBankDev &b, const int32_t *sets, int set_size, const float *logits, size_t S,
                                      size_t n_new, float score_ref10, int calc_avg, float threshold, float avg_threshold, float *agg, float *avg,
                                      int32_t *label) {
    const size_t rows = S * (size_t)set_size, blocks = (rows * n_new + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_score_set_stream_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b, sets, logits, rows, n_new, score_ref10, calc_avg,
                       threshold, avg_threshold, agg, avg, label);
    return hipGetLastError();
}

}  // namespace rp
