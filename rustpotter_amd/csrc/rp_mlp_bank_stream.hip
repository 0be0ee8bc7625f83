// rp_mlp_bank_stream.hip -- the wakeword-model forward of a LIVE batch over a model bank (rp_stream_batch_new_model_bank): the logits of
// every stream's new windows with that stream's OWN model bank[stream_model[s]].  mlp_bank_stream_kernel and the window means it corrects
// with (window_means_bank_stream_kernel).  DESIGN.md §4.4.
//
// ARITHMETIC: row by row that of mlp_mfma_kernel<NT, kMlpBf16x3> in window mode (rp_mlp.hip), which the shared-model live batches and
// rp_mlp_forward_windows take for fewer than 32 windows a stream -- so a window's logits are a function of its frames and its model alone:
// not of the batch, of the stream's place in it, or of how the caller cuts the audio into calls.  The row's own window mean leaves each
// feature as it is loaded (f - mu), the difference is split into three bf16 parts (mlp_split_bf16x3), the k-blocks of 32 run in ascending
// order up to kpad (the zero-padded blocks too: they add products of zeros, as they do there), lane (li, lk) holds k = 32 u + 8 lk .. + 8, and
// every block and 16-output tile gets six v_mfma_f32_16x16x32_bf16 in the order x0 w2, x1 w1, x2 w0, x0 w1, x1 w0, x0 w0; then bias, ReLU
// where tail layers follow, and mlp_tail_layers<4>.  An output of a matrix instruction depends on its own row of A alone, so how rows are
// grouped into tiles changes nothing.
//
// WEIGHTS: no second image and no staging in LDS.  ModelBankDev::wimg is MlpDev::wwin3, [frame f][part p][k-half h][32 outputs] in 16-byte
// pieces, and holds the very values of the w1t planes mlp_mfma_kernel stages: the B fragment of block u, part p, output o for lane lk is
// piece ((f 3 + p) 2 + h) 32 + o with f = 2 u + (lk >> 1), h = lk & 1 -- sixteen lanes read 256 contiguous bytes; pieces with f >= L are
// zeros (kept in registers: the image ends at L).  The fragments and the rows' features are loaded kBsAhead blocks ahead.
//
// SHAPE: one wave (= one workgroup) owns up to RT = 1 or 2 tiles of 16 new windows of ONE stream, so a fragment loaded once serves up to
// 32 rows; a call of more than 16 RT new windows has further waves per stream.  Rows behind the stream's count are computed on its last
// row and dropped; a wave whose stream has no model (index outside [0, W)) writes zero rows and leaves.  The second 16-output tile is
// skipped, wave-uniformly, for a model whose layer 1 is at most 16 wide.  The tail weights are read where they lie (at most 2 x 33 x 32
// floats, the same address for the 16 lanes of a phase): with a model per wave there is nobody to share an LDS copy with.
//
// COST MODEL (NOT MEASURED here; tools/bench_stream_model_bank.py measures): with one model per stream nothing is shared between streams.
// A call reads every connected stream's layer-1 image once, L(s) x 3 072 bytes -- 599 KB at L = 195 -- against 16 (L + n) x 4 bytes of
// frames and 6 x 2 matrix instructions per block and row tile: the image traffic binds, not the matrix pipe.  Streams that share a model
// share only what the caches keep.  <1> is built for three waves per SIMD (at most 168 registers), <2> for two: its two blocks in flight
// and the one at the matrix instructions are 3 x 40 registers of operands.
#include "rp_mlp_bank_stream.h"
#include "rp_host.h"

namespace rp {

// window means of every stream's new windows at its own window length: the same sums in frame order as window_means_kernel, hence the same
// bits.  The frame rows are the batch's (cap frames a stream); the window that ends at the first new frame `fill` starts L(s) - 1 frames
// before it.  mean [S][n_new][16]; rows of a stream without a model are not written (nobody reads them).
__global__ __launch_bounds__(256) void window_means_bank_stream_kernel(ModelBankDev b, const int32_t *__restrict__ stream_model,
                                                                       const float *__restrict__ frames, size_t cap, size_t fill, size_t n_new,
                                                                       unsigned tiles, float *__restrict__ mean) {
    const size_t s = blockIdx.x / tiles;
    const size_t w0 = (size_t)(blockIdx.x - s * tiles) * 64;
    const int mi = stream_model[s];
    if (mi < 0 || mi >= b.W) return;
    const int L = b.e[mi].L;
    const size_t nw = n_new - w0 < 64 ? n_new - w0 : 64;
    window_means_body(frames + (s * cap + fill - (size_t)(L - 1) + w0) * 16, (int)nw, L, 16, mean + (s * n_new + w0) * 16);
}

template <int RT>
__global__ __launch_bounds__(64, RT == 1 ? 3 : 2) void mlp_bank_stream_kernel(ModelBankDev bank, const int32_t *__restrict__ stream_model,
                                                             const float *__restrict__ frames, size_t cap, size_t fill, int n_new, unsigned wps,
                                                             const float *__restrict__ mean, float *__restrict__ out) {
    __shared__ float h1[16 * kBsH1], h2[16 * kBsH1];
    const size_t s = blockIdx.x / wps;
    const int r0 = (int)(blockIdx.x - (unsigned)s * wps) * (16 * RT);   // first new window of this wave
    const int rows_here = n_new - r0 < 16 * RT ? n_new - r0 : 16 * RT;
    const int label_pitch = bank.label_pitch;
    float *orow = out + (s * (size_t)n_new + (size_t)r0) * (size_t)label_pitch;
    const int mi = stream_model[s];
    if (mi < 0 || mi >= bank.W) {   // no model: zero rows
        for (int i = threadIdx.x; i < rows_here * label_pitch; i += 64) orow[i] = 0.f;
        return;
    }
    const ModelBankEntry e = bank.e[mi];
    // the frame the stream's first new window starts at: e.L - 1 frames before the first new frame
    mlp_bank_stream_body<RT>(bank, e, frames + (s * cap + fill - (size_t)(e.L - 1)) * 16, mean + s * (size_t)n_new * 16,
                             out + s * (size_t)n_new * (size_t)label_pitch, n_new, r0, h1, h2);
}

hipError_t launch_window_means_bank_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *stream_model, const float *frames, size_t S,
                                           size_t cap, size_t fill, size_t n_new, float *mean) {
    if (S == 0 || n_new == 0 || b.W == 0) return hipSuccess;
    if (max_L < 1 || max_L > 256 || fill + 1 < (size_t)max_L || fill + n_new > cap) return hipErrorInvalidValue;   // every window lies inside its row
    const size_t tiles = (n_new + 63) / 64, blocks = tiles * S;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = ((n_new < 64 ? n_new : 64) + (size_t)max_L - 1) * 16 * sizeof(float);
    hipLaunchKernelGGL(window_means_bank_stream_kernel, dim3((unsigned)blocks), dim3(256), lds, st, b, stream_model, frames, cap, fill, n_new,
                       (unsigned)tiles, mean);
    return hipGetLastError();
}

hipError_t launch_mlp_bank_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *stream_model, const float *frames, size_t S,
                                  size_t cap, size_t fill, size_t n_new, const float *mean, float *logits) {
    if (S == 0 || n_new == 0 || b.W == 0 || b.label_pitch == 0) return hipSuccess;
    if (max_L < 1 || fill + 1 < (size_t)max_L || fill + n_new > cap || n_new > 0x7fffffffULL) return hipErrorInvalidValue;
    const int rt = n_new > 16 ? 2 : 1;
    const size_t wps = (n_new + 16 * rt - 1) / (16 * rt);
    if (S * wps > 0x7fffffffULL) return hipErrorInvalidValue;
    if (rt == 1)
        hipLaunchKernelGGL(mlp_bank_stream_kernel<1>, dim3((unsigned)(S * wps)), dim3(64), 0, st, b, stream_model, frames, cap, fill, (int)n_new,
                           (unsigned)wps, mean, logits);
    else
        hipLaunchKernelGGL(mlp_bank_stream_kernel<2>, dim3((unsigned)(S * wps)), dim3(64), 0, st, b, stream_model, frames, cap, fill, (int)n_new,
                           (unsigned)wps, mean, logits);
    return hipGetLastError();
}

}  // namespace rp
