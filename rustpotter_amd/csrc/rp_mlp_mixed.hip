// rp_mlp_mixed.hip -- the model side of a live-stream batch over MIXED sets (rp_stream_batch_new_mixed_sets): the fronts of
// rp_mlp_model_set.hip's live kernels with the COMBINED Lmax(s) -- the longest window over the live slots of the stream's reference row and
// model row, read from the per-stream table of stream_targets_kernel -- in the place of the model row's own.  The first window of a call
// starts Lmax(s) - 1 frames before the first new frame for every slot; slot j reads L_j frames from there.  The bodies are shared
// (window_means_body, rp_mlp_windows.h; mlp_bank_stream_body, rp_mlp_bank_stream.h); nn_score_set_stream_kernel does not read Lmax and is
// reused as it is.
#include "rp_mlp_bank_stream.h"
#include "rp_mlp_windows.h"
#include "rp_host.h"

namespace rp {

// window_means_set_stream_kernel with the combined Lmax(s): mean [S][set_size][n_new][16]; rows of empty slots are not written
__global__ __launch_bounds__(256) void window_means_mixed_stream_kernel(ModelBankDev b, const int32_t *__restrict__ sets, int set_size,
                                                                        const BankWakeword *__restrict__ table, const float *__restrict__ frames,
                                                                        size_t cap, size_t fill, size_t n_new, unsigned tiles,
                                                                        float *__restrict__ mean) {
    const size_t row = blockIdx.x / tiles;
    const size_t w0 = (size_t)(blockIdx.x - row * tiles) * 64;
    const size_t s = row / (size_t)set_size;
    const int mi = sets[row];
    if (mi < 0 || mi >= b.W) return;
    const int lmax = table[s].max_len;
    const size_t nw = n_new - w0 < 64 ? n_new - w0 : 64;
    window_means_body(frames + (s * cap + fill - (size_t)(lmax - 1) + w0) * 16, (int)nw, b.e[mi].L, 16, mean + (row * n_new + w0) * 16);
}

// mlp_set_stream_kernel<RT> with the combined Lmax(s): logits [S][set_size][n_new][label_pitch], every row written (an empty slot: zeros)
template <int RT>
__global__ __launch_bounds__(64, RT == 1 ? 3 : 2) void mlp_mixed_stream_kernel(ModelBankDev bank, const int32_t *__restrict__ sets, int set_size,
                                                                               const BankWakeword *__restrict__ table,
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
    const int lmax = table[s].max_len;
    const ModelBankEntry e = bank.e[mi];
    mlp_bank_stream_body<RT>(bank, e, frames + (s * cap + fill - (size_t)(lmax - 1)) * 16, mean + row * (size_t)n_new * 16, out_s, n_new, r0, h1, h2);
}

// max_L: the bank's longest model window (the staging); max_window: the longest window any stream of the batch may have, the combined
// history + 1 -- every window lies inside its row
hipError_t launch_window_means_mixed_stream(hipStream_t st, const ModelBankDev &b, int max_L, int max_window, const int32_t *sets, int set_size,
                                            const BankWakeword *table, const float *frames, size_t S, size_t cap, size_t fill, size_t n_new,
                                            float *mean) {
    if (S == 0 || n_new == 0 || b.W == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords || !table) return hipErrorInvalidValue;
    if (max_L < 1 || max_L > 256 || max_window < max_L || fill + 1 < (size_t)max_window || fill + n_new > cap) return hipErrorInvalidValue;
    const size_t tiles = (n_new + 63) / 64, blocks = tiles * S * (size_t)set_size;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = ((n_new < 64 ? n_new : 64) + (size_t)max_L - 1) * 16 * sizeof(float);
    hipLaunchKernelGGL(window_means_mixed_stream_kernel, dim3((unsigned)blocks), dim3(256), lds, st, b, sets, set_size, table, frames, cap, fill, n_new,
                       (unsigned)tiles, mean);
    return hipGetLastError();
}

hipError_t launch_mlp_mixed_stream(hipStream_t st, const ModelBankDev &b, int max_L, int max_window, const int32_t *sets, int set_size,
                                   const BankWakeword *table, const float *frames, size_t S, size_t cap, size_t fill, size_t n_new,
                                   const float *mean, float *logits) {
    if (S == 0 || n_new == 0 || b.W == 0 || b.label_pitch == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords || !table) return hipErrorInvalidValue;
    if (max_L < 1 || max_window < max_L || fill + 1 < (size_t)max_window || fill + n_new > cap || n_new > 0x7fffffffULL) return hipErrorInvalidValue;
    const int rt = n_new > 16 ? 2 : 1;
    const size_t wps = (n_new + 16 * rt - 1) / (16 * rt), blocks = S * (size_t)set_size * wps;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    if (rt == 1)
        hipLaunchKernelGGL(mlp_mixed_stream_kernel<1>, dim3((unsigned)blocks), dim3(64), 0, st, b, sets, set_size, table, frames, cap, fill, (int)n_new,
                           (unsigned)wps, mean, logits);
    else
        hipLaunchKernelGGL(mlp_mixed_stream_kernel<2>, dim3((unsigned)blocks), dim3(64), 0, st, b, sets, set_size, table, frames, cap, fill, (int)n_new,
                           (unsigned)wps, mean, logits);
    return hipGetLastError();
}

}  // namespace rp
