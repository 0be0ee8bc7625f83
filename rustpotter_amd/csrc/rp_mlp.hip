// rp_mlp.hip -- the wakeword model: forward (src/wakewords/nn/wakeword_nn.rs:101-163,305-389; mlp_layer_kernel,
// mlp_mfma_kernel on the matrix cores, normalize_windows_batch_kernel), its route (mlp_route, mlp_forward), scoring and training
// (wakeword_model_train.rs:204-209).  The staged-frame kernels are in rp_mlp_windows.hip, the streaming one in rp_mlp_stream.hip, the live
// model bank's in rp_mlp_bank_stream.hip.
// DESIGN.md §4.4.
#include "rp_mlp_dev.h"
#include "rp_host.h"

namespace rp {

// -------------------------------------------------------------------------- MLP
// Linear (x.W^T + b, W [out][in]) + optional ReLU, f32, k-ordered accumulation like
// candle's CPU gemm restated in the oracle.  One wave per (row, 64 outputs) tile with
// the input row staged in LDS.  (Round-1 correctness path; profiles/HISTORY.md lists the MFMA
// bf16 path for BASELINE config 5 as next.)
__global__ __launch_bounds__(64) void mlp_layer_kernel(const float *__restrict__ x, size_t B, int in, int on,
                                                       const float *__restrict__ Wt, const float *__restrict__ bias,
                                                       int relu, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xr = reinterpret_cast<float *>(smem);
    const size_t b = blockIdx.x;
    const int o = blockIdx.y * 64 + threadIdx.x;
    for (int i = threadIdx.x; i < in; i += 64) xr[i] = x[b * in + i];
    __syncthreads();
    if (o >= on) return;
    const float *w = Wt + (size_t)o * in;
    float s = 0.f;
    for (int i = 0; i < in; ++i) s += xr[i] * w[i];
    s += bias[o];
    if (relu && s < 0.f) s = 0.f;
    out[b * on + o] = s;
}

// MfccNormalizer::normalize of the windows of many streams, one window per block: row = s * n_win + w, rows first_row .. of the call
__global__ __launch_bounds__(64) void normalize_windows_batch_kernel(const float *__restrict__ mfcc, size_t frame_pitch, size_t n_win,
                                                                      size_t first_row, int L, int K, float *__restrict__ x) {
    const size_t row = first_row + blockIdx.x;
    const size_t s = row / n_win, w = row - s * n_win;
    const float *src = mfcc + (s * frame_pitch + w) * K;
    float *dst = x + (size_t)blockIdx.x * L * K;
    for (int k = threadIdx.x; k < K; k += 64) {
        float sum = 0.f;
        for (int i = 0; i < L; ++i) sum += src[(size_t)i * K + k];
        for (int i = 0; i < L; ++i) dst[(size_t)i * K + k] = src[(size_t)i * K + k] - sum / (float)L;
    }
}

hipError_t launch_normalize_windows_batch(hipStream_t st, const float *mfcc, size_t frame_pitch, size_t n_win, size_t first_row,
                                          size_t n_rows, int L, int K, float *x) {
    if (n_rows == 0) return hipSuccess;
    if (n_rows > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(normalize_windows_batch_kernel, dim3((unsigned)n_rows), dim3(64), 0, st, mfcc, frame_pitch, n_win, first_row, L, K, x);
    return hipGetLastError();
}

// windows first_win .. first_win + n_win of ONE run of frames: a single stream of first_win + n_win windows
hipError_t launch_normalize_windows(hipStream_t st, const float *mfcc, size_t first_win, size_t n_win, int L, int K,
                                    float *x) {
    return launch_normalize_windows_batch(st, mfcc, 0, first_win + n_win, first_win, n_win, L, K, x);
}

// (nn_score_row, a window's label, score and average score, is in rp_mlp_dev.h: rp_mlp_model_set.hip shares it)
__global__ __launch_bounds__(256) void nn_score_kernel(const float *__restrict__ logits, size_t n_rows, int nl, int none_index,
                                                       float ref, int calc_avg, float threshold, float avg_threshold,
                                                       float *__restrict__ agg, float *__restrict__ avg, int32_t *__restrict__ label,
                                                       uint32_t *__restrict__ hot, size_t rows_per_stream) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    float score, av;
    int bi;
    nn_score_row(logits + r * nl, nl, none_index, ref, calc_avg, threshold, avg_threshold, &score, &av, &bi);
    agg[r] = score; avg[r] = av; label[r] = bi;
    // a stream with no window that passed cannot fire (detector.rs:411-429): the scan skips it (every writer stores the same value)
    if (hot && score != -2.f) hot[r / rows_per_stream] = 1u;
}

// The same where stream s runs its own model of a bank: label count and none_index come from the model of the row's stream, rows are
// [S][win_pitch] with logits label_pitch floats apart.  A row that is no window of its stream can never fire.
__global__ __launch_bounds__(256) void nn_score_bank_kernel(ModelBankDev b, const int32_t *__restrict__ stream_model, const float *__restrict__ logits,
                                                            size_t S, size_t n_frames, size_t win_pitch, float ref, int calc_avg, float threshold,
                                                            float avg_threshold, float *__restrict__ agg, float *__restrict__ avg,
                                                            int32_t *__restrict__ label, uint32_t *__restrict__ hot) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= S * win_pitch) return;
    const size_t s = r / win_pitch, w = r - s * win_pitch;
    const int mi = stream_model[s];
    float score = -2.f, av = 0.f;
    int bi = -1;
    if (mi >= 0 && mi < b.W) {
        const ModelBankEntry e = b.e[mi];
        if (n_frames >= (size_t)e.L && w < n_frames - (size_t)e.L + 1)
            nn_score_row(logits + r * (size_t)b.label_pitch, e.n_labels, e.none_index, ref, calc_avg, threshold, avg_threshold, &score, &av, &bi);
    }
    agg[r] = score; avg[r] = av; label[r] = bi;
    if (hot && score != -2.f) hot[s] = 1u;
}

hipError_t launch_nn_score_bank(hipStream_t st, const ModelBankDev &b, const int32_t *stream_model, const float *logits, size_t S, size_t n_frames,
                                size_t win_pitch, float score_ref10, int calc_avg, float threshold, float avg_threshold, float *agg, float *avg,
                                int32_t *label, uint32_t *hot) {
    const size_t blocks = (S * win_pitch + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_score_bank_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b, stream_model, logits, S, n_frames, win_pitch, score_ref10,
                       calc_avg, threshold, avg_threshold, agg, avg, label, hot);
    return hipGetLastError();
}

// The same over the new windows of a live call (rp_stream_batch_new_model_bank): rows [S][n_new], every one a window of its stream
__global__ __launch_bounds__(256) void nn_score_bank_stream_kernel(ModelBankDev b, const int32_t *__restrict__ stream_model, const float *__restrict__ logits,
                                                                   size_t S, size_t n_new, float ref, int calc_avg, float threshold, float avg_threshold,
                                                                   float *__restrict__ agg, float *__restrict__ avg, int32_t *__restrict__ label) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= S * n_new) return;
    const int mi = stream_model[r / n_new];
    float score = -2.f, av = 0.f;
    int bi = -1;
    if (mi >= 0 && mi < b.W) {
        const ModelBankEntry e = b.e[mi];
        nn_score_row(logits + r * (size_t)b.label_pitch, e.n_labels, e.none_index, ref, calc_avg, threshold, avg_threshold, &score, &av, &bi);
    }
    agg[r] = score; avg[r] = av; label[r] = bi;
}

hipError_t launch_nn_score_bank_stream(hipStream_t st, const ModelBankDev &b, const int32_t *stream_model, const float *logits, size_t S, size_t n_new,
                                       float score_ref10, int calc_avg, float threshold, float avg_threshold, float *agg, float *avg, int32_t *label) {
    const size_t blocks = (S * n_new + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_score_bank_stream_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b, stream_model, logits, S, n_new, score_ref10, calc_avg,
                       threshold, avg_threshold, agg, avg, label);
    return hipGetLastError();
}

// the label of every detection's window, gathered behind the scan; 0 behind a stream's detections, as rp_batch_detect_model leaves them
__global__ __launch_bounds__(256) void model_bank_labels_kernel(const BatchDetection *__restrict__ det, const int32_t *__restrict__ n_det,
                                                                const int32_t *__restrict__ label, size_t S, size_t win_pitch, int max_det,
                                                                int32_t *__restrict__ det_label) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= S * (size_t)max_det) return;
    const size_t s = i / (size_t)max_det;
    const int j = (int)(i - s * (size_t)max_det);
    int32_t v = 0;
    if (j < n_det[s]) {
        const int32_t w = det[i].window;
        if (w >= 0 && (size_t)w < win_pitch) v = label[s * win_pitch + (size_t)w];
    }
    det_label[i] = v;
}

hipError_t launch_model_bank_labels(hipStream_t st, const BatchDetection *det, const int32_t *n_det, const int32_t *label, size_t S, size_t win_pitch,
                                    int max_det, int32_t *det_label) {
    if (S == 0 || max_det <= 0) return hipSuccess;
    const size_t blocks = (S * (size_t)max_det + 255) / 256;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(model_bank_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, st, det, n_det, label, S, win_pitch, max_det, det_label);
    return hipGetLastError();
}

hipError_t launch_nn_score(hipStream_t st, const float *logits, size_t n_rows, int n_labels, int none_index, float score_ref10,
                           int calc_avg, float threshold, float avg_threshold, float *agg, float *avg, int32_t *label, uint32_t *hot,
                           size_t rows_per_stream) {
    if (n_rows == 0) return hipSuccess;
    if (hot && rows_per_stream == 0) return hipErrorInvalidValue;
    const size_t blocks = (n_rows + 255) / 256;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nn_score_kernel, dim3((unsigned)blocks), dim3(256), 0, st, logits, n_rows, n_labels, none_index, score_ref10, calc_avg,
                       threshold, avg_threshold, agg, avg, label, hot, rows_per_stream);
    return hipGetLastError();
}

// mlp_layer_kernel layer after layer; layer l writes dst_of(l)
template <class DstOf>
static hipError_t launch_mlp_layers(hipStream_t st, const float *x, size_t B, int n_layers, const int *dims, float *const *W,
                                    float *const *Bv, DstOf dst_of) {
    if (B == 0) return hipSuccess;
    const float *cur = x;
    for (int l = 0; l < n_layers; ++l) {
        float *dst = dst_of(l);
        dim3 grid((unsigned)B, (unsigned)((dims[l + 1] + 63) / 64));
        size_t lds = (size_t)dims[l] * sizeof(float);
        if (lds > 64 * 1024) return hipErrorInvalidValue;
        hipLaunchKernelGGL(mlp_layer_kernel, grid, dim3(64), lds, st, cur, B, dims[l], dims[l + 1], W[l], Bv[l],
                           l + 1 < n_layers ? 1 : 0, dst);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        cur = dst;
    }
    return hipSuccess;
}

// the forward: hidden layers through the two scratch buffers in turn
static hipError_t launch_mlp(hipStream_t st, const float *x, size_t B, int n_layers, const int *dims, float *const *W,
                             float *const *Bv, float *scratch0, float *scratch1, float *out) {
    float *bufs[2] = {scratch0, scratch1};
    return launch_mlp_layers(st, x, B, n_layers, dims, W, Bv, [&](int l) { return l + 1 == n_layers ? out : bufs[l & 1]; });
}

// ------------------------------------------------------------------ MLP training
// WakewordModelTrain's loop (src/wakewords/nn/wakeword_model_train.rs:204-209): full-batch forward,
// log_softmax + nll (mean over the batch), backward, plain SGD.  The matrices are tiny (tens of recordings x a few
// thousand features): one thread per result element, reductions along the batch / the layer width in a loop.  The forward is
// mlp_layer_kernel's, every layer's output kept (launch_train_forward).

// per row: log_softmax (x - max - ln(sum exp(x - max))), loss_row = -log_sm[label], dlogits = (softmax - onehot) / B
__global__ __launch_bounds__(64) void train_softmax_grad_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels,
                                                                size_t B, int C, float *__restrict__ dz, float *__restrict__ loss_rows) {
    const size_t b = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    train_softmax_row(logits + b * C, labels[b], B, C, dz + b * C, loss_rows + b);
}

// dZprev[b][i] = A_prev[b][i] > 0 ? sum_o dZ[b][o] * W[o][i] : 0     (ReLU backward through the layer's input)
__global__ __launch_bounds__(256) void train_backprop_kernel(const float *__restrict__ dz, const float *__restrict__ W,
                                                             const float *__restrict__ a_prev, size_t B, int in, int on,
                                                             float *__restrict__ dz_prev) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t b = blockIdx.y;
    if (i >= in) return;
    float s = 0.f;
    for (int o = 0; o < on; ++o) s += dz[b * on + o] * W[(size_t)o * in + i];
    dz_prev[b * in + i] = a_prev[b * in + i] > 0.f ? s : 0.f;
}

// SGD step of one layer: W[o][i] -= lr * sum_b dZ[b][o] * A_in[b][i];  bias[o] -= lr * sum_b dZ[b][o]
__global__ __launch_bounds__(256) void train_update_kernel(const float *__restrict__ dz, const float *__restrict__ a_in, size_t B,
                                                           int in, int on, float lr, float *__restrict__ W, float *__restrict__ bias) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int o = blockIdx.y;
    if (i > in) return;  // i == in: the bias column
    float g = 0.f;
    if (i < in) {
        for (size_t b = 0; b < B; ++b) g += dz[b * on + o] * a_in[b * in + i];
        W[(size_t)o * in + i] = W[(size_t)o * in + i] - g * lr;
    } else {
        for (size_t b = 0; b < B; ++b) g += dz[b * on + o];
        bias[o] = bias[o] - g * lr;
    }
}

hipError_t launch_train_forward(hipStream_t st, const float *x, size_t B, int n_layers, const int *dims, float *const *W,
                                float *const *Bv, float *const *act) {
    return launch_mlp_layers(st, x, B, n_layers, dims, W, Bv, [&](int l) { return act[l]; });
}

// act[l] = output of layer l (post-ReLU for hidden layers, logits for the last); dz[l] same shapes
hipError_t launch_train_step(hipStream_t st, const float *x, const int32_t *labels, size_t B, int n_layers, const int *dims,
                             float *const *W, float *const *Bv, float *const *act, float *const *dz, float lr, float *loss_rows) {
    if (B == 0) return hipSuccess;
    hipError_t e = launch_train_forward(st, x, B, n_layers, dims, W, Bv, act);
    if (e != hipSuccess) return e;
    const int C = dims[n_layers];
    hipLaunchKernelGGL(train_softmax_grad_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, act[n_layers - 1], labels, B, C,
                       dz[n_layers - 1], loss_rows);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (int l = n_layers - 1; l >= 0; --l) {
        const int in = dims[l], on = dims[l + 1];
        const float *a_in = l == 0 ? x : act[l - 1];
        if (l > 0) {  // through W_l as it was in the forward pass, before its own update
            hipLaunchKernelGGL(train_backprop_kernel, dim3((unsigned)((in + 255) / 256), (unsigned)B), dim3(256), 0, st, dz[l], W[l],
                               act[l - 1], B, in, on, dz[l - 1]);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(train_update_kernel, dim3((unsigned)((in + 1 + 255) / 256), (unsigned)on), dim3(256), 0, st, dz[l], a_in, B, in,
                           on, lr, W[l], Bv[l]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ MLP on MFMA
// One workgroup = 8 waves = 128 rows; one wave = one 16-row tile x all layer-1 outputs (NT
// 16-column tiles).  The layer-1 weights are walked in k-groups of 128: the group's [16*NT][128]
// slice is staged once per workgroup in LDS and shared by the 8 waves (reading it per wave from L2
// cost more than the HBM stream itself: 0.39 -> 0.18 ms when removed), rows stream from HBM in
// the MFMA A-operand layout (16 rows x 64 B per instruction; 5.5 TB/s measured on its own).
//  f32 variant:  v_mfma_f32_16x16x4_f32, exact f32 (each output is a k-ordered fmaf chain).  A lane
//                loads 16 bytes of its row per 16-k block and feeds component j to MFMA step j; the
//                weight lane does the same, so both sides agree on the (permuted) k order.
//  bf16 variant: v_mfma_f32_16x16x32_bf16, inputs rounded to bf16 (RNE) in registers, f32 accumulate.
// The tail layers (<= 130 x 32 weights) run per row from LDS.  HBM-bound by construction: 4*in bytes
// per row against 2*in*N1 flops (12 480 B/row, ceiling 0.64 G rows/s at 8 TB/s).
constexpr int kMlpWaves = 8;
constexpr int kMlpRowsPerWave = 16;
constexpr int kMlpKG = 128;  // k-group staged per step

__host__ __device__ constexpr int mlp_wpitch_f32() { return kMlpKG + 4; }   // floats per staged weight row
__host__ __device__ constexpr int mlp_wpitch_bf16() { return kMlpKG + 8; }  // bf16 per staged weight row

template <int NT, int PREC>
__global__ __launch_bounds__(64 * kMlpWaves, 3) void mlp_mfma_kernel(
    const float *__restrict__ x, size_t B, int in, int kpad, const float *__restrict__ w1f,
    const __bf16 *__restrict__ w1h, const float *__restrict__ b1, const float *__restrict__ tail, int tail_floats,
    int n_layers, int d1, int d2, int d3, int d4, int h2w, int wbuf_floats, float *__restrict__ out, size_t row_stride,
    size_t rows_per_stream, size_t stream_skip, const float *__restrict__ mean, const float *__restrict__ wsum, int K, uint32_t *redo,
    int redo_list) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int N1P = 16 * NT;
    // redo (rp_kernels.h, kMlpF16x2): kMlpF16x2 lists the rows that hold a feature beyond the f16 range (redo[0] = rows listed, from
    // redo[2] on their indices); redo_list != 0: this launch computes exactly those rows (the f32 matrix instructions) and the last
    // workgroup to leave puts redo[0] and redo[1] back to zero
    const uint32_t *rlist = nullptr;
    if (redo_list) {
        const size_t n = redo[0];
        if (n == 0) return;   // nothing listed (every call on ordinary features): no workgroup touches the counters
        if ((size_t)blockIdx.x * kMlpWaves * kMlpRowsPerWave >= n) {   // the whole workgroup: nothing (more) listed
            if (threadIdx.x == 0 && atomicAdd(redo + 1, 1u) == gridDim.x - 1) { redo[0] = 0; redo[1] = 0; }
            return;
        }
        B = n;
        rlist = redo + 2;
    }
    auto row_of = [&](size_t i) -> size_t { return rlist ? (size_t)rlist[i] : i; };   // position in this launch -> row of x / out
    float *tl = reinterpret_cast<float *>(smem);                       // tail weights
    float *wbuf = tl + ((tail_floats + 3) & ~3);                       // staged weight group; later h1 [waves][16][N1P+1]
    float *h2_all = wbuf + wbuf_floats;                                // [waves][16][h2w]
    for (int i = threadIdx.x; i < tail_floats; i += blockDim.x) tl[i] = tail[i];

    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int li = l & 15, lk = l >> 4;
    const size_t row0 = ((size_t)blockIdx.x * kMlpWaves + wave) * kMlpRowsPerWave;
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    size_t r = row0 + li;
    if (r >= B) r = B - 1;  // rows past the end recompute the last row; their results are dropped
    r = row_of(r);
    // row_stride != 0: rows are overlapping windows read in place from the frame array (MlpForward::windows)
    const float *xr = row_stride ? x + r * row_stride + (r / rows_per_stream) * stream_skip : x + r * in;
    float rng = 0.f;   // kMlpF16x2: largest |feature| this lane has seen

    // staged weight groups are double buffered when they fit (NT <= 2): the next group's global
    // loads are issued before this group's MFMAs and land in the other buffer, one barrier per group
    constexpr bool DB = NT <= 2;
    constexpr int PF = mlp_wpitch_f32(), PH = mlp_wpitch_bf16();
    // 16-byte pieces of a staged weight group: f32 four k each, bf16 eight, kMlpF16x2 eight in each of its two planes
    constexpr int NPL = PREC == kMlpBf16x3 ? 3 : 2;   // planes of a split form's weights: w1h = [NPL][N1P][kpad] (MlpDev::w1t / w1s)
    constexpr int NPIECE = PREC == kMlpF32 ? N1P * (kMlpKG / 4) : PREC == kMlpBf16 ? N1P * (kMlpKG / 8) : NPL * N1P * (kMlpKG / 8);
    constexpr int NV = (NPIECE + 64 * kMlpWaves - 1) / (64 * kMlpWaves);
    const int half = DB ? wbuf_floats / 2 : 0;
    // every thread moves NV pieces; when the slice is a whole number of pieces per thread the bounds test is dropped
    // (a conditional store into wreg makes the compiler keep the array in scratch memory)
    constexpr bool FULL = NPIECE % (64 * kMlpWaves) == 0;
    // one 16-byte piece = 4 f32 or 8 bf16; plain vector values (HIP's float4 struct is copied with memcpy, which keeps
    // the staging array in scratch memory)
    auto wload = [&](int g, f32x4 (&wreg)[NV]) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int i = threadIdx.x + v * 64 * kMlpWaves;
            if (PREC == kMlpF32) {
                const int o = i / (kMlpKG / 4), c = i - o * (kMlpKG / 4);
                if (FULL || o < N1P) wreg[v] = *reinterpret_cast<const f32x4 *>(w1f + (size_t)o * kpad + g * kMlpKG + 4 * c);
            } else if (PREC == kMlpBf16) {
                const int o = i / (kMlpKG / 8), c = i - o * (kMlpKG / 8);
                if (FULL || o < N1P) wreg[v] = *reinterpret_cast<const f32x4 *>(w1h + (size_t)o * kpad + g * kMlpKG + 8 * c);
            } else {   // kMlpF16x2: plane p of w1h = [2][N1P][kpad] f16 (MlpDev::w1s)
                const int po = i / (kMlpKG / 8), c = i - po * (kMlpKG / 8);
                if (FULL || po < NPL * N1P) wreg[v] = *reinterpret_cast<const f32x4 *>(w1h + (size_t)po * kpad + g * kMlpKG + 8 * c);
            }
        }
    };
    auto wstore = [&](float *dstbuf, const f32x4 (&wreg)[NV]) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int i = threadIdx.x + v * 64 * kMlpWaves;
            if (PREC == kMlpF32) {
                const int o = i / (kMlpKG / 4), c = i - o * (kMlpKG / 4);
                if (FULL || o < N1P) *reinterpret_cast<f32x4 *>(dstbuf + o * PF + 4 * c) = wreg[v];
            } else if (PREC == kMlpBf16) {
                const int o = i / (kMlpKG / 8), c = i - o * (kMlpKG / 8);
                if (FULL || o < N1P) *reinterpret_cast<f32x4 *>(reinterpret_cast<__bf16 *>(dstbuf) + o * PH + 8 * c) = wreg[v];
            } else {   // both planes, rows po = plane * N1P + o at the bf16 pitch
                const int po = i / (kMlpKG / 8), c = i - po * (kMlpKG / 8);
                if (FULL || po < NPL * N1P) *reinterpret_cast<f32x4 *>(reinterpret_cast<__bf16 *>(dstbuf) + po * PH + 8 * c) = wreg[v];
            }
        }
    };
    const int ngrp = kpad / kMlpKG;
    // the rows of k-group g+1 are requested before the MFMAs of group g (registers double buffered like the staged
    // weights), so the HBM stream never drains at the per-group barrier
    constexpr int NA = PREC == kMlpF32 ? kMlpKG / 16 : 2 * (kMlpKG / 32);
    float4 areg[2][NA];
    // Windows (mean != nullptr): the row's own window mean leaves each feature as it is loaded -- MfccNormalizer::normalize itself.  For
    // mfcc_size 16 a lane's pieces always hold the same coefficients (k0 mod 16 = 4 lk, or 8 (lk & 1) + 4 (u & 1)): registers; for the
    // other sizes (multiples of 4) the piece's place in the frame, kc = k0 mod K, is carried from group to group and the four means come
    // from the row's mean vector (a cached 16-byte load).  Until round 4 the mean was taken out after layer 1
    // (W.(f - mu) = W.f - sum_k mu[k] wsum[k]): real MFCCs sit on offsets many times their spread, and a sum that carries the offsets loses
    // their size in f32 rounding (5e-6 of a score on the reference's own recording).
    const bool norm = mean != nullptr, norm16 = norm && K == 16;
    float4 mu_a = make_float4(0.f, 0.f, 0.f, 0.f), mu_b = mu_a;
    const float *mrow = norm ? mean + r * (size_t)K : nullptr;
    int kc[NA];
    const int kstep = (norm && !norm16) ? kMlpKG % K : 0;
#pragma unroll
    for (int u = 0; u < NA; ++u) kc[u] = 0;
    if (norm16) {
        const float4 *mu = reinterpret_cast<const float4 *>(mrow);
        if (PREC == kMlpF32) mu_a = mu[lk];
        else { mu_a = mu[2 * (lk & 1)]; mu_b = mu[2 * (lk & 1) + 1]; }
    } else if (norm) {
#pragma unroll
        for (int u = 0; u < NA; ++u) kc[u] = (PREC == kMlpF32 ? 16 * u + 4 * lk : 32 * (u >> 1) + 8 * lk + 4 * (u & 1)) % K;
    }
    auto aload = [&](int g, float4 (&dst)[NA]) __attribute__((always_inline)) {   // called for g = 0, 1, 2, .. in this order
        const int kg = g * kMlpKG;
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            // f32: piece u = k-step u (16 wide), lane part 4*lk;  bf16: pieces 2u / 2u+1 = low / high half of the lane's 8
            const int k0 = PREC == kMlpF32 ? kg + 16 * u + 4 * lk : kg + 32 * (u >> 1) + 8 * lk + 4 * (u & 1);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + 3 < in) {
                v = *reinterpret_cast<const float4 *>(xr + k0);
                if (norm) {
                    const float4 m = norm16 ? ((PREC == kMlpF32 || !(u & 1)) ? mu_a : mu_b) : *reinterpret_cast<const float4 *>(mrow + kc[u]);
                    v.x -= m.x; v.y -= m.y; v.z -= m.z; v.w -= m.w;
                }
            }
            dst[u] = v;
            if (norm && !norm16) { kc[u] += kstep; if (kc[u] >= K) kc[u] -= K; }
        }
    };
    {
        f32x4 w0[NV];
        wload(0, w0);
        aload(0, areg[0]);
        wstore(wbuf, w0);
    }
    __syncthreads();  // group 0 staged (and the tail weights landed)
    auto group = [&](int g, float4 (&a)[NA], float4 (&anext)[NA]) __attribute__((always_inline)) {
        const float *cur = wbuf + ((DB && (g & 1)) ? half : 0);
        // The next group's requests go out after the first k-step of this one: that step waits for this group's rows
        // (requested one group ago) while nothing newer is outstanding, so the wait never covers the new requests.
        f32x4 wnext[NV];
        auto prefetch = [&]() __attribute__((always_inline)) { if (g + 1 < ngrp) { wload(g + 1, wnext); aload(g + 1, anext); } };
        if (PREC == kMlpF32) {
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                float4 b[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) b[n] = *reinterpret_cast<const float4 *>(cur + (16 * n + li) * PF + 16 * u + 4 * lk);
                // the accumulators take turns so that consecutive MFMAs do not wait on each other's result
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[n].x, acc[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[n].y, acc[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[n].z, acc[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[n].w, acc[n], 0, 0, 0);
                if (u == 0) prefetch();
            }
        } else if (PREC == kMlpF16x2) {
            // f16 two-way splits: x0 = rtz_f16(x) (as f32: 13 mantissa bits cleared), x1 = rtz_f16(x - x0); x0 w0 + x1 w0 + x0 w1
            // on the f16 matrix instruction, f32 accumulate.  A row with a feature beyond the f16 range is listed and computed again by the
            // f32 matrix instructions (one v_max_f32 |x| per feature finds it).
            const __bf16 *wb = reinterpret_cast<const __bf16 *>(cur);
#pragma unroll
            for (int u = 0; u < NA / 2; ++u) {
                const float4 lo = a[2 * u], hi = a[2 * u + 1];
                const float xs[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                u32x4 h0, h1;
                mlp_split_f16x2(xs, h0, h1, rng);
                const f16x8 av0 = __builtin_bit_cast(f16x8, h0), av1 = __builtin_bit_cast(f16x8, h1);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const f16x8 b0 = *reinterpret_cast<const f16x8 *>(wb + (16 * n + li) * PH + 32 * u + 8 * lk);
                    const f16x8 b1v = *reinterpret_cast<const f16x8 *>(wb + (N1P + 16 * n + li) * PH + 32 * u + 8 * lk);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av0, b0, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av1, b0, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av0, b1v, acc[n], 0, 0, 0);
                }
                if (u == 0) prefetch();
            }
        } else if (PREC == kMlpBf16x3) {
            // three bf16 parts per operand (exact), six of the nine partial products, f32 accumulate: f32-grade (RP_MLP_F32; rp_mlp_stream.hip
            // has the same arithmetic).  No range limit: nothing is listed.
            const __bf16 *wb = reinterpret_cast<const __bf16 *>(cur);
#pragma unroll
            for (int u = 0; u < NA / 2; ++u) {
                const float4 lo = a[2 * u], hi = a[2 * u + 1];
                const float xs[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                u32x4 h0, h1, h2;
                mlp_split_bf16x3(xs, h0, h1, h2);
                const bf16x8 av0 = __builtin_bit_cast(bf16x8, h0), av1 = __builtin_bit_cast(bf16x8, h1), av2 = __builtin_bit_cast(bf16x8, h2);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const bf16x8 b0 = *reinterpret_cast<const bf16x8 *>(wb + (16 * n + li) * PH + 32 * u + 8 * lk);
                    const bf16x8 b1v = *reinterpret_cast<const bf16x8 *>(wb + (N1P + 16 * n + li) * PH + 32 * u + 8 * lk);
                    const bf16x8 b2v = *reinterpret_cast<const bf16x8 *>(wb + (2 * N1P + 16 * n + li) * PH + 32 * u + 8 * lk);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av0, b2v, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av1, b1v, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av2, b0, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av0, b1v, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av1, b0, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av0, b0, acc[n], 0, 0, 0);
                }
                if (u == 0) prefetch();
            }
        } else {
            const __bf16 *wb = reinterpret_cast<const __bf16 *>(cur);
#pragma unroll
            for (int u = 0; u < NA / 2; ++u) {
                const float4 lo = a[2 * u], hi = a[2 * u + 1];
                bf16x8 av;
                av[0] = (__bf16)lo.x; av[1] = (__bf16)lo.y; av[2] = (__bf16)lo.z; av[3] = (__bf16)lo.w;
                av[4] = (__bf16)hi.x; av[5] = (__bf16)hi.y; av[6] = (__bf16)hi.z; av[7] = (__bf16)hi.w;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const bf16x8 b = *reinterpret_cast<const bf16x8 *>(wb + (16 * n + li) * PH + 32 * u + 8 * lk);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b, acc[n], 0, 0, 0);
                }
                if (u == 0) prefetch();
            }
        }
        if (g + 1 < ngrp) {
            if (!DB) __syncthreads();  // single buffer: everyone must be done reading before the overwrite
            wstore(wbuf + ((DB && !(g & 1)) ? half : 0), wnext);
        }
        __syncthreads();
    };
    for (int g = 0; g < ngrp; g += 2) {
        group(g, areg[0], areg[1]);
        if (g + 1 < ngrp) group(g + 1, areg[1], areg[0]);
    }
    // every wave is past the last barrier, i.e. done with the staged weights: the buffer becomes h1
    // ---- layer-1 bias (+ReLU) -> LDS, C/D layout: col = lane&15, row = (lane>>4)*4 + reg
    float *h1 = wbuf + wave * kMlpRowsPerWave * (N1P + 1);
    const bool relu1 = n_layers > 1;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = acc[n][e];
            v += b1[16 * n + li];
            if (relu1 && v < 0.f) v = 0.f;
            h1[(4 * lk + e) * (N1P + 1) + 16 * n + li] = v;
        }
    wave_lds_sync();
    // ---- tail layers: lane = (row l&15, output phase l>>4), outputs strided by 4 over the phases
    {
        const int rr = l & 15, ph = l >> 4;
        const bool row_ok = row0 + rr < B;
        const size_t orow = row_ok ? row_of(row0 + rr) : 0;
        if (PREC == kMlpF16x2) {   // the four lanes (row rr, k part 0..3) of a row agree on its range; one of them lists it
            rng = fmaxf(rng, __shfl_xor(rng, 16));
            rng = fmaxf(rng, __shfl_xor(rng, 32));
            if (ph == 0 && row_ok && !(rng <= 65504.f)) mlp_redo_append(redo, (uint32_t)orow, B);
        }
        const int dd[5] = {in, d1, d2, d3, d4};
        mlp_tail_layers<4>(tl, n_layers, d1, d2, d3, d4, h1 + rr * (N1P + 1), h2_all + (wave * kMlpRowsPerWave + rr) * h2w, ph, row_ok,
                           out + orow * (size_t)dd[n_layers], [](int i) { return i; }, [] { wave_lds_sync(); });
    }
    if (redo_list) {
        __syncthreads();
        if (threadIdx.x == 0 && atomicAdd(redo + 1, 1u) == gridDim.x - 1) { redo[0] = 0; redo[1] = 0; }
    }
}

// The route of one forward (mlp_route): decided once per call from the model, the request and the tuning variables; the launchers read it.
// kind: mlp_layer_kernel per layer, mlp_mfma_kernel on dense rows, mlp_stream_kernel, mlp_windows_kernel, mlp_windows_wide_kernel,
// mlp_mfma_kernel reading the windows in place
enum MlpKind { kMlpLayers, kMlpRows, kMlpStream, kMlpWindows, kMlpWindowsWide, kMlpInPlace };
struct MlpRoute {
    MlpKind kind = kMlpLayers;
    int prec = kMlpF32;          // the operand form (PREC; the window kernels' P3 = kMlpBf16x3)
    bool redo = false;           // kMlpF16x2: the listed rows follow with mlp_mfma_kernel<NT, kMlpF32>
    MlpStreamPlan plan;          // kMlpStream
    // mlp_mfma_kernel (the call's kernel or its second pass): LDS bytes, the staged weight group(s) and an h2 row in floats
    size_t lds = 0, wbuf = 0;
    int h2w = 1;
    WinRoute win;                // the staged-frame kernels (rp_mlp_dev.h)
    std::string report;          // what ran (Ctx::last_mlp_kernel); empty for the per-layer kernel, which leaves it as it is
};

// LDS of mlp_mfma_kernel in form prec: the tail weights; the staged layer-1 weight group(s) -- 16 NT rows x the bf16 pitch, in floats, for
// the two f16 planes of kMlpF16x2 (f32 and bf16 groups are smaller; the three bf16 planes of kMlpBf16x3 take half again as much), double
// buffered at NT <= 2 -- which later hold h1; and h2 [waves][16][h2w]
static size_t mlp_mfma_lds(const MlpDev &m, int prec, int *h2w, size_t *wbuf) {
    static_assert(mlp_wpitch_bf16() >= mlp_wpitch_f32(), "staged weight group");
    *h2w = 1;
    for (int l2 = 2; l2 < m.n_layers; ++l2) *h2w = std::max(*h2w, m.dims[l2] + 1);
    *h2w |= 1;
    *wbuf = std::max((size_t)(prec == kMlpBf16x3 ? 24 : 16) * m.nt * mlp_wpitch_bf16() * (m.nt <= 2 ? 2 : 1),
                     (size_t)kMlpWaves * kMlpRowsPerWave * (16 * m.nt + 1));
    *wbuf = (*wbuf + 3) & ~(size_t)3;
    return ((size_t)((m.tail_floats + 3) & ~3) + *wbuf + (size_t)kMlpWaves * kMlpRowsPerWave * *h2w) * sizeof(float);
}

// wide hidden layers do not fit the CU's 160 KB and take the per-layer kernel instead (Model::create)
bool mlp_mfma_fits(const MlpDev &m) {
    int h2w;
    size_t wbuf;
    return mlp_mfma_lds(m, kMlpF32, &h2w, &wbuf) <= 160 * 1024;
}

// mlp_mfma_kernel<NT, PREC> over B rows (in-place windows: row = s * n_win + w, K floats apart, a new stream skips the rest of its row);
// redo_list: only the rows listed in redo
template <int NT, int PREC>
static hipError_t launch_mlp_pass(hipStream_t st, const MlpDev &m, const MlpRoute &r, const MlpForward &q, size_t B, const void *w1h,
                                  uint32_t *redo, int redo_list) {
    const size_t blocks = (B + kMlpWaves * kMlpRowsPerWave - 1) / (kMlpWaves * kMlpRowsPerWave);
    hipLaunchKernelGGL((mlp_mfma_kernel<NT, PREC>), dim3((unsigned)blocks), dim3(64 * kMlpWaves), r.lds, st, q.x, B, m.dims[0], m.kpad, m.w1f,
                       static_cast<const __bf16 *>(w1h), m.b1, m.tail, m.tail_floats, m.n_layers, m.dims[1], m.dims[2], m.dims[3], m.dims[4],
                       r.h2w, (int)r.wbuf, q.out, q.windows ? (size_t)q.K : 0, q.windows ? q.n_win : 1,
                       q.windows ? (q.frame_pitch - q.n_win) * q.K : 0, q.mean, q.wsum, q.K, redo, redo_list);
    return hipGetLastError();
}

// the route's mlp_mfma_kernel passes: the call itself (dense rows, windows in place), then the rows its split form listed
template <int NT>
static hipError_t launch_mlp_nt(hipStream_t st, const MlpDev &m, const MlpRoute &r, const MlpForward &q, size_t B, uint32_t *redo) {
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(mlp_mfma_kernel<NT, kMlpBf16>), 160 * 1024); e != hipSuccess) return e;
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(mlp_mfma_kernel<NT, kMlpF32>), 160 * 1024); e != hipSuccess) return e;
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(mlp_mfma_kernel<NT, kMlpF16x2>), 160 * 1024); e != hipSuccess) return e;
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(mlp_mfma_kernel<NT, kMlpBf16x3>), 160 * 1024); e != hipSuccess) return e;
    if (B > 0xffffffffULL || r.lds > 160 * 1024) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (r.kind == kMlpRows || r.kind == kMlpInPlace) {
        switch (r.prec) {
        case kMlpBf16: e = launch_mlp_pass<NT, kMlpBf16>(st, m, r, q, B, m.w1h, nullptr, 0); break;
        case kMlpF16x2: e = launch_mlp_pass<NT, kMlpF16x2>(st, m, r, q, B, m.w1s, redo, 0); break;
        case kMlpBf16x3: e = launch_mlp_pass<NT, kMlpBf16x3>(st, m, r, q, B, m.w1t, nullptr, 0); break;
        default: e = launch_mlp_pass<NT, kMlpF32>(st, m, r, q, B, m.w1h, nullptr, 0);
        }
    }
    // sized for every row: workgroups past the list's end leave at once
    if (e == hipSuccess && r.redo) e = launch_mlp_pass<NT, kMlpF32>(st, m, r, q, B, m.w1h, redo, 1);
    return e;
}

static hipError_t launch_mlp_mfma(hipStream_t st, const MlpDev &m, const MlpRoute &r, const MlpForward &q, size_t B, uint32_t *redo) {
    switch (m.nt) {
    case 1: return launch_mlp_nt<1>(st, m, r, q, B, redo);
    case 2: return launch_mlp_nt<2>(st, m, r, q, B, redo);
    case 5: return launch_mlp_nt<5>(st, m, r, q, B, redo);
    case 9: return launch_mlp_nt<9>(st, m, r, q, B, redo);
    }
    return hipErrorInvalidValue;
}

static MlpRoute mlp_route(Model &md, const MlpForward &q) {
    MlpRoute r;
    if (!md.mfma_ok) return r;
    const MlpDev &m = md.dev;
    // RP_MLP_F32: three bf16 parts; RP_MLP_F32_FAST: two f16 parts (+ the listed rows with the f32 matrix instructions); RP_MLP_F32_STRICT: the
    // f32 matrix instructions; RP_MLP_BF16: bf16 inputs -- for dense rows only (it permits bf16 inputs: the windows take RP_MLP_F32's form)
    r.prec = q.precision == RP_MLP_F32_FAST ? kMlpF16x2 : q.precision == RP_MLP_F32_STRICT ? kMlpF32
             : (q.precision == RP_MLP_BF16 && !q.windows) ? kMlpBf16 : kMlpBf16x3;
    r.redo = r.prec == kMlpF16x2;
    if (q.windows) {
        // whole streams (or long runs of windows): the staged-frame kernels, the frames staged once per workgroup -- mfcc_size 16, layer 1
        // <= 32 (mlp_windows_kernel) or <= 144 (mlp_windows_wide_kernel, five output tiles; Model::create has no matrix-core form beyond
        // 144, md.mfma_ok above) wide, the tail layers <= 32, windows of 2 .. 256 frames.  A window of ONE frame is its own mean: every
        // normalised feature is exactly 0, and only mlp_mfma_kernel, which subtracts the row's own mean as it loads, keeps that; staged about
        // another window's mean, W.(f - c) and the correction (mu - c).wsum are two roundings of one quantity, and what they leave is
        // measured against logits that carry no feature at all (2.2 x the 1e-5 gate, tests/test_gpu_mlp_windows_builds.py)
        int form = 0;
        if (r.prec != kMlpF32 && (r.prec == kMlpBf16x3 ? m.wwin3 : m.wwin) && q.K == 16 && m.dims[0] % 16 == 0 && m.dims[1] <= 144 &&
            q.n_win >= 32 && m.dims[0] / 16 >= 2 && m.dims[0] / 16 <= 256 && m.tail_floats <= 6144) {
            form = m.dims[1] <= 32 ? 1 : 2;
            for (int l2 = 2; l2 <= m.n_layers; ++l2) if (m.dims[l2] > 32) form = 0;
            if (const char *env = std::getenv("RP_MLP_WINDOWS")) if (env[0] == '0') form = 0;
        }
        r.kind = form == 1 ? kMlpWindows : form == 2 ? kMlpWindowsWide : kMlpInPlace;
        const size_t tiles = (q.n_win + kWinTile - 1) / kWinTile;
        if (form == 1) {
            // tiles per workgroup: as few workgroups per stream as 7 tiles each allow, the tiles spread evenly over them
            static const int cap_env = std::getenv("RP_MLP_WIN_TILES") ? std::atoi(std::getenv("RP_MLP_WIN_TILES")) : kWinMaxTiles;   // experiments
            r.win.tiles = mlp_windows_cut(q.n_win, cap_env >= 1 && cap_env <= kWinMaxTiles ? cap_env : kWinMaxTiles).tiles;
        } else if (form == 2) {
            // 2 or 4 (measured per 8 192 streams x 202 windows, Medium / Large: 7 tiles 3.87 / 8.62 ms at two waves per SIMD, 4 tiles
            // 3.36 / 7.90 at four, 2 tiles 3.84 / 11.2 -- the weights once per 64 rows)
            const size_t wgs = (tiles + 3) / 4;
            r.win.tiles = (tiles + wgs - 1) / wgs <= 2 ? 2 : 4;
            r.win.nq = (m.dims[1] + 31) / 32;
        }
        if (form) {
            r.win.bps = (q.n_win + r.win.tiles * kWinTile - 1) / (r.win.tiles * kWinTile);
            r.win.slots = mlp_windows_slots(r.win.tiles, m.dims[0] / 16);
            r.win.lds = mlp_windows_lds(m.tail_floats, r.win.slots, r.win.tiles, r.prec == kMlpBf16x3 ? 3 : 2, r.win.nq);
        }
    } else {
        // RP_MLP_STREAM (a tuning knob of benchmarks and tests, not an arithmetic switch): 0 = mlp_mfma_kernel for every shape, 2 = the
        // streaming kernel for RP_MLP_F32_STRICT too -- by default the f32 matrix rate binds there, and mlp_mfma_kernel's 24 waves per CU
        // overlap it better (0.198 against 0.207 ms at BASELINE C5); the other forms stream at the HBM rate (bf16 0.132 against 0.155 ms)
        const char *e = std::getenv("RP_MLP_STREAM");
        const int mode = e ? (e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1) : 1;
        const bool stream = q.allow_stream && mode != 0 && (r.prec != kMlpF32 || mode == 2) && mlp_stream_supported(m, q.x, r.prec) &&
                            md.stream_plan(q.x, q.B, r.prec, &r.plan);
        r.kind = stream ? kMlpStream : kMlpRows;
    }
    // a model whose three-part weight groups do not fit the CU's LDS beside its tail layers (the widest ones) runs the f32 matrix
    // instructions instead: exact either way
    const bool mfma = r.kind == kMlpRows || r.kind == kMlpInPlace;
    r.lds = mlp_mfma_lds(m, mfma ? r.prec : kMlpF32, &r.h2w, &r.wbuf);
    if (mfma && r.prec == kMlpBf16x3 && r.lds > 160 * 1024) r.lds = mlp_mfma_lds(m, r.prec = kMlpF32, &r.h2w, &r.wbuf);
    static const char *const name[] = {"", "mlp_mfma_kernel", "mlp_stream_kernel", "mlp_windows_kernel", "mlp_windows_wide_kernel", "mlp_mfma_kernel"};
    r.report = std::string(name[r.kind]) + (r.prec == kMlpF32 ? "<f32 matrix instructions>" : r.prec == kMlpBf16 ? "<bf16>" : r.prec == kMlpF16x2 ? "<f16x2 splits>" : "<bf16x3 splits>");
    if (r.kind == kMlpInPlace) r.report += r.redo ? ", windows read in place," : ", windows read in place";
    if (r.redo) r.report += " + mlp_mfma_kernel<f32> on listed rows";
    return r;
}

bool mlp_forward(Ctx &c, const MlpForward &q) {
    Model &md = *q.m;
    const MlpDev &m = md.dev;
    const size_t rows = q.windows ? q.S * q.n_win : q.B;
    if (q.timed) c.time_begin(kKernelMlp);
    const MlpRoute r = mlp_route(md, q);
    uint32_t *redo = r.kind == kMlpLayers ? nullptr : c.mlp_redo(rows);
    hipError_t e = (r.kind != kMlpLayers && !redo) ? hipErrorOutOfMemory : hipSuccess;
    const char *build = "";   // mlp_stream_kernel: the build a launch knob chose, where it is not the default one
    if (e == hipSuccess && rows) {
        switch (r.kind) {
        case kMlpLayers:
            e = launch_mlp(c.stream, q.x, rows, (int)md.dims.size() - 1, md.dims.data(), md.W.data(), md.B.data(), q.scratch[0], q.scratch[1], q.out);
            break;
        case kMlpStream: e = launch_mlp_stream(c.stream, m, r.plan, q.x, rows, r.prec, q.out, c.n_cu, redo, &build); break;
        case kMlpWindows:
        case kMlpWindowsWide:
            if (rows > 0xffffffffULL || r.win.bps * q.S > 0x7fffffffULL || r.win.lds > 160 * 1024) e = hipErrorInvalidValue;
            else e = (r.kind == kMlpWindows ? launch_mlp_windows : launch_mlp_windows_wide)(c.stream, m, r.win, q, r.prec == kMlpBf16x3, redo);
            break;
        default: break;
        }
        // dense rows and windows in place, and the second pass of the split form
        if (e == hipSuccess && (r.kind == kMlpRows || r.kind == kMlpInPlace || r.redo)) e = launch_mlp_mfma(c.stream, m, r, q, rows, redo);
        // a failure between the split pass and the pass over the listed rows must not leave rows of THIS call listed for the next one:
        // the two counter words go back to zero behind whatever was queued, as dtw_abort does for the DTW words
        if (e != hipSuccess && redo) (void)hipMemsetAsync(redo, 0, 2 * sizeof(uint32_t), c.stream);
    }
    if (e == hipSuccess && q.report && !r.report.empty()) c.last_mlp_kernel = r.report + build;
    if (q.timed) c.time_end();
    return hip_ok(e, r.kind == kMlpLayers ? "mlp_layer_kernel" : "mlp_mfma_kernel");
}

}  // namespace rp
