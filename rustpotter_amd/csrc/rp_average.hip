// rp_average.hip -- enrolment on the device: MfccNormalizer::normalize over whole samples (src/mfcc/wav_file_extractor.rs:67) and
// MfccAverager::average (src/mfcc/averager.rs:5-37) with the unbanded Dtw::compute_optimal_path / retrieve_optimal_path
// (src/mfcc/dtw.rs:11-55,106-138) over MfccComparator::calculate_distance (src/mfcc/comparator.rs:28-48), for many wakewords per launch.
// Both kernels restate the host code of rp_builder.cpp (compute_wav_mfccs, average_step) operation for operation -- the same f32
// multiplies, adds, square roots and divisions in the same order (-ffp-contract=off: nothing is fused) -- so that a batch gives the
// bytes the single call gives.
#include "rp_device.h"

namespace rp {

// ------------------------------------------------------------------ normalise
// One workgroup per sample: raw [S][frame_pitch][K] frames of the batched MFCC launch, of which sample s owns the first nf[s]; the
// normalised rows go to out + dst_row[s] * K (the call's templates, concatenated in fold order).  A thread owns whole columns: the
// column sum runs over the frames in order, as the host's.
__global__ __launch_bounds__(64) void normalize_samples_kernel(const float *__restrict__ raw, size_t frame_pitch, int K,
                                                               const int32_t *__restrict__ nf, const int64_t *__restrict__ dst_row,
                                                               float *__restrict__ out) {
    const size_t s = blockIdx.x;
    const int n = nf[s];
    const float *src = raw + s * frame_pitch * (size_t)K;
    float *dst = out + (size_t)dst_row[s] * (size_t)K;
    for (int j = threadIdx.x; j < K; j += 64) {
        float sum = 0.f;
        for (int i = 0; i < n; ++i) sum += src[(size_t)i * K + j];
        const float mean = sum / (float)n;
        for (int i = 0; i < n; ++i) dst[(size_t)i * K + j] = src[(size_t)i * K + j] - mean;
    }
}

hipError_t launch_normalize_samples(hipStream_t st, const float *raw, size_t S, size_t frame_pitch, int K, const int32_t *nf,
                                    const int64_t *dst_row, float *out) {
    if (S == 0) return hipSuccess;
    if (S > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(normalize_samples_kernel, dim3((unsigned)S), dim3(64), 0, st, raw, frame_pitch, K, nf, dst_row, out);
    return hipGetLastError();
}

// -------------------------------------------------------------------- average
// A workgroup folds one wakeword at a time (the grid strides over the listed wakewords): template 0 is the origin [m][K], every further
// template [n][K] updates it in place.  Per fold:
//   1. squared norms of the origin rows and of the frames (each once per fold: dot_a / dot_b do not depend on the partner);
//   2. all m x n cell costs 1 - dot_ab / sqrt(dot_a * dot_b), independent of each other, into the matrix;
//   3. the recurrence D[r][c] = cost + min(min(min(inf, D[r-1][c]), D[r][c-1]), D[r-1][c-1]) one anti-diagonal at a time (the first row
//      and column are the prefix sums of the same sweep);
//   4. the back-trace, one thread, at most m + n - 2 moves by construction.  A warping path is monotone, so the positions it pushes for
//      origin row x are one run of consecutive frames ylo[x]..yhi[x]: that is all the mean needs;
//   5. the mean: row x = (origin[x] + frames[ylo] + .. + frames[yhi] (+ min(m-1, n-1) more copies of frames[0] for row 0: the zero
//      pairs the reference's path vector starts with, which its reversal puts LAST)) / count, summed in that order.
// LDS: origin and frames with an odd row pitch, the norms, the runs, and -- kLdsMatrix -- the matrix with an even row pitch (an
// anti-diagonal then strides by an odd number of words: no bank is hit twice).  Otherwise the matrix is the workgroup's slice of `ws`.
constexpr int kAvgThreads = 256;

__host__ __device__ inline int avg_row_pitch(int K) { return K | 1; }
__host__ __device__ inline int avg_matrix_pitch(int n) { return (n + 1) & ~1; }

size_t average_lds_bytes(int m, int n, int K, bool lds_matrix) {
    return sizeof(float) * ((size_t)(m + n) * avg_row_pitch(K) + 3 * (size_t)m + (size_t)n + (lds_matrix ? average_matrix_floats(m, n) : 0));
}
size_t average_matrix_floats(int m, int n) { return (size_t)m * avg_matrix_pitch(n); }

template <bool kLdsMatrix>
__global__ __launch_bounds__(kAvgThreads) void average_kernel(AverageBatch b, const int32_t *__restrict__ list, unsigned n_list,
                                                              float *__restrict__ ws, size_t ws_slice) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = b.K, KP = avg_row_pitch(K), tid = threadIdx.x;
    for (unsigned li = blockIdx.x; li < n_list; li += gridDim.x) {
        const int w = list[li];
        const int t0 = b.first[w], T = b.count[w];
        const int m = b.lens[t0];
        int n_max = 1;
        for (int f = 1; f < T; ++f) n_max = max(n_max, b.lens[t0 + f]);
        float *og = reinterpret_cast<float *>(smem);   // [m][KP]
        float *fr = og + (size_t)m * KP;               // [n_max][KP]
        float *na = fr + (size_t)n_max * KP;           // [m]
        float *nb = na + m;                            // [n_max]
        int *ylo = reinterpret_cast<int *>(nb + n_max);  // [m]
        int *yhi = ylo + m;                            // [m]
        float *D;
        if constexpr (kLdsMatrix) D = reinterpret_cast<float *>(yhi + m);
        else D = ws + (size_t)blockIdx.x * ws_slice;
        {
            const float *src = b.feats + (size_t)b.row_off[t0] * K;
            for (int i = tid; i < m * K; i += kAvgThreads) { const int x = i / K; og[x * KP + (i - x * K)] = src[i]; }
        }
        for (int f = 1; f < T; ++f) {
            const int n = b.lens[t0 + f], P = avg_matrix_pitch(n);
            const float *src = b.feats + (size_t)b.row_off[t0 + f] * K;
            for (int i = tid; i < n * K; i += kAvgThreads) { const int y = i / K; fr[y * KP + (i - y * K)] = src[i]; }
            __syncthreads();   // origin (loaded, or the previous fold's mean) and frames are in place
            for (int i = tid; i < m + n; i += kAvgThreads) {
                const float *v = i < m ? og + i * KP : fr + (i - m) * KP;
                float dot = 0.f;
                for (int k = 0; k < K; ++k) dot += v[k] * v[k];
                if (i < m) { na[i] = dot; ylo[i] = n; yhi[i] = -1; }
                else nb[i - m] = dot;
            }
            __syncthreads();
            for (int i = tid; i < m * n; i += kAvgThreads) {
                const int r = i / n, c = i - r * n;
                const float *a = og + r * KP, *x = fr + c * KP;
                float dot_ab = 0.f;
                for (int k = 0; k < K; ++k) dot_ab += a[k] * x[k];
                const float magnitude = sqrtf(na[r] * nb[c]);
                D[(size_t)r * P + c] = 1.f - (magnitude == 0.f ? 0.f : dot_ab / magnitude);
            }
            __syncthreads();
            for (int d = 0; d <= m + n - 2; ++d) {
                const int r_lo = d - (n - 1) > 0 ? d - (n - 1) : 0, r_hi = d < m - 1 ? d : m - 1;
                for (int r = r_lo + tid; r <= r_hi; r += kAvgThreads) {
                    const int c = d - r;
                    float *cell = D + (size_t)r * P + c;
                    float prev;
                    if (r > 0 && c > 0) prev = fminf(fminf(fminf(RP_INF, cell[-P]), cell[-1]), cell[-P - 1]);
                    else if (r > 0) prev = cell[-P];
                    else if (c > 0) prev = cell[-1];
                    else continue;   // D[0][0] is its cost
                    *cell = *cell + prev;
                }
                __syncthreads();
            }
            if (tid == 0) {
                int r = m - 1, c = n - 1;
                for (int step = m + n - 2; step > 0 && (r > 0 || c > 0); --step) {
                    if (r > 0 && c > 0) {
                        const float *cell = D + (size_t)r * P + c;
                        const float ins = cell[-P], del = cell[-1], mat = cell[-P - 1];
                        const float mn = fminf(fminf(fminf(RP_INF, ins), del), mat);
                        if (mn == mat) { --r; --c; }
                        else if (mn == ins) --r;
                        else if (mn == del) --c;
                        else { --r; --c; }   // no comparison holds (every neighbour NaN): the host would not return; any move does
                    } else if (r > 0) --r;
                    else --c;
                    ylo[r] = c;                    // within a row the pushed positions run towards column 0
                    if (yhi[r] < 0) yhi[r] = c;
                }
            }
            __syncthreads();
            const int extra = m - 1 < n - 1 ? m - 1 : n - 1;
            for (int i = tid; i < m * K; i += kAvgThreads) {
                const int x = i / K, k = i - x * K;
                float sum = og[x * KP + k];
                int count = 1;
                for (int y = ylo[x]; y <= yhi[x]; ++y) { sum += fr[y * KP + k]; ++count; }
                if (x == 0) for (int e = 0; e < extra; ++e) { sum += fr[k]; ++count; }
                og[x * KP + k] = sum / (float)count;
            }
            __syncthreads();   // the frames are free for the next template, the origin is whole
        }
        // (a thread stores the elements it loaded, or -- after a fold -- what the barrier above made whole)
        float *dst = b.avg + (size_t)b.out_row[w] * K;
        for (int i = tid; i < m * K; i += kAvgThreads) { const int x = i / K; dst[i] = og[x * KP + (i - x * K)]; }
        __syncthreads();   // before the next wakeword's origin overwrites this one
    }
}

hipError_t launch_average(hipStream_t st, const AverageBatch &b, const int32_t *list, size_t n_list, bool lds_matrix, size_t lds_bytes,
                          unsigned blocks, float *ws, size_t ws_slice) {
    if (n_list == 0) return hipSuccess;
    if (blocks == 0 || n_list > 0x7fffffffULL || lds_bytes > 160 * 1024 || (!lds_matrix && !ws)) return hipErrorInvalidValue;
    const void *fn = lds_matrix ? reinterpret_cast<const void *>(average_kernel<true>) : reinterpret_cast<const void *>(average_kernel<false>);
    if (lds_bytes > 64 * 1024)
        if (hipError_t e = allow_dynamic_lds(fn, 160 * 1024); e != hipSuccess) return e;
    if (lds_matrix) hipLaunchKernelGGL(average_kernel<true>, dim3(blocks), dim3(kAvgThreads), lds_bytes, st, b, list, (unsigned)n_list, ws, ws_slice);
    else hipLaunchKernelGGL(average_kernel<false>, dim3(blocks), dim3(kAvgThreads), lds_bytes, st, b, list, (unsigned)n_list, ws, ws_slice);
    return hipGetLastError();
}

}  // namespace rp
