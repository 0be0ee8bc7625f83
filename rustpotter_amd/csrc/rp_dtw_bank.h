// rp_dtw_bank.h -- the per-lane DTW walks of the wakeword-bank kernels, shared by rp_dtw_bank.hip (one wakeword per stream) and rp_dtw_set.hip
// (a set of wakewords per stream): bank_dtw, bank_chk_window, bank_dtw_ref.  Device code only; include behind rp_device.h.
#pragma once
#include "rp_device.h"

namespace rp {

// One DTW of the lane's window against one template of L rows (m == n == L: the window is cut to the template's length keeping the oldest
// frames), with the arithmetic of the register kernels of rp_dtw.hip OPERATION FOR OPERATION -- sequential column sums / L, unit-length frame by
// rsqrtf of the fma-chained squared norm, d = fmaf(-a[k], y[k], d) chained from 1, v = d + min3, cost / (m + n), dtw_logistic -- so that a
// window gets the bits it gets from dtw_band_kernel / dtw_band2_kernel / dtw_band_wide_kernel.  The form is dtw_band_wide_kernel's with one
// template: the ring of the 2W unit-length frames inside the band as register pairs, two band cells per packed FMA, the template row a
// wave-uniform read (scalar loads), rows unrolled 2W at a time so that every ring slot and band index is a compile-time register.
// chk: max over the frames loaded of (squared norm, its reciprocal square root) -- the norm-range test of those kernels, same columns.
template <int K, int W, int KP>
__device__ __forceinline__ float bank_dtw(const float *xl, int L, const float *__restrict__ rows, float score_ref, float &chk_out) {
    constexpr int B = 2 * W;
    constexpr int MEAN_UNROLL = K <= 5 ? 10 : 4;   // frames in flight per wait, as the register kernels
    // MfccNormalizer::normalize, src/mfcc/normalizer.rs:17-29: sequential column sums
    float mu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = 0.f;
#pragma unroll MEAN_UNROLL
    for (int i = 0; i < L; ++i) {
#pragma unroll
        for (int k = 0; k < K; ++k) mu[k] += xl[i * KP + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = mu[k] / (float)L;

    v2f ring[B / 2][K];  // ring[j][k] = { y_slot(2j)[k], y_slot(2j+1)[k] }
#pragma unroll
    for (int j = 0; j < B / 2; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) ring[j][k] = (v2f){0.f, 0.f};

    float chk = 0.f;
#define RP_LOAD_COL(c, slot)                                                              \
    do {                                                                                  \
        float y_[K], bb_ = 0.f;                                                           \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                   \
            y_[k] = xl[((c)-1) * KP + k] - mu[k];                                         \
            bb_ = fmaf(y_[k], y_[k], bb_);                                                \
        }                                                                                 \
        const float inv_ = bb_ > 0.f ? rsqrtf(bb_) : 0.f;                                 \
        chk = fmaxf(fmaxf(chk, inv_), bb_);                                               \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                   \
            if (((slot)&1) == 0) ring[(slot) / 2][k].x = y_[k] * inv_;                    \
            else ring[(slot) / 2][k].y = y_[k] * inv_;                                    \
        }                                                                                 \
    } while (0)

#pragma unroll
    for (int c = 1; c < W; ++c) RP_LOAD_COL(c, c % B);

    // P[q] = D[r-1][(r-1-W)+q]; row 0 has D[0][0] = 0 at q = W
    float P[B + 1];
#pragma unroll
    for (int q = 0; q <= B; ++q) P[q] = RP_INF;
    P[W] = 0.f;

    // columns c > n are never read back by an in-range cell and stay unguarded, as in the register kernels (the stage holds W frames of slack)
#define RP_ROWS(GUARD)                                                                                 \
    _Pragma("unroll") for (int u = 0; u < B; ++u) {                                                    \
        const int r = r0 + u;                                                                          \
        if (r < L) { /* rows 1..m-1 only: row m is never read (dtw.rs:101) */                          \
            RP_LOAD_COL(r + W - 1, (u + W) % B);                                                       \
            const float *arow = rows + (size_t)(r - 1) * K;                                            \
            v2f dd[B / 2];                                                                             \
            _Pragma("unroll") for (int j = 0; j < B / 2; ++j) dd[j] = (v2f){1.f, 1.f};                 \
            _Pragma("unroll") for (int k = 0; k < K; ++k) {                                            \
                const v2f a2 = (v2f){arow[k], arow[k]};                                                \
                _Pragma("unroll") for (int j = 0; j < B / 2; ++j)                                      \
                    dd[j] = __builtin_elementwise_fma(-a2, ring[j][k], dd[j]);                         \
            }                                                                                          \
            float left = RP_INF;                                                                       \
            _Pragma("unroll") for (int q = 0; q < B; ++q) {                                            \
                const int slot = (1 + u + q + B - W) % B;                                              \
                const float d = (slot & 1) ? dd[slot / 2].y : dd[slot / 2].x;                          \
                float v = d + fminf(fminf(P[q + 1], left), P[q]);                                      \
                if (GUARD) v = (r - W + q >= 1) ? v : RP_INF;                                          \
                P[q] = v;                                                                              \
                left = v;                                                                              \
            }                                                                                          \
        }                                                                                              \
    }

    {
        const int r0 = 1;
        RP_ROWS(true)
    }
    for (int r0 = 1 + B; r0 < L; r0 += B) { RP_ROWS(false) }
#undef RP_ROWS
#undef RP_LOAD_COL
    chk_out = chk;
    return dtw_logistic(P[W + 1] / (float)(L + L), score_ref);   // D[m-1][n] for m == n
}

// chk of bank_dtw over the window's own L frames only (the same sums, the same fma chain): what dtw_generic_kernel tests, which loads no frame
// behind the window's end.  For wakewords past the register kernels' staging (BankWakeword::window_chk), and only once a lane was flagged.
template <int K, int KP>
__device__ __noinline__ float bank_chk_window(const float *xl, int L) {
    float mu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = 0.f;
    for (int i = 0; i < L; ++i) {
#pragma unroll
        for (int k = 0; k < K; ++k) mu[k] += xl[i * KP + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = mu[k] / (float)L;
    float chk = 0.f;
    for (int i = 0; i < L; ++i) {
        float bb = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float y = xl[i * KP + k] - mu[k];
            bb = fmaf(y, y, bb);
        }
        const float inv = bb > 0.f ? rsqrtf(bb) : 0.f;
        chk = fmaxf(fmaxf(chk, inv), bb);
    }
    return chk;
}

// The same DTW with the reference-shaped cell of dtw_ref_kernel (comparator.rs:28-48: three sequential dot products of the template row AS
// GIVEN and the mean-normalised frame, one sqrt, one divide), for windows with a frame outside kDtwNormLo..kDtwFixLimit and wakewords with a
// row outside kDtwNormLo..kDtwNormHiRow.  Band in LDS, lane-minor; the whole wave walks it, the lanes that need it keep the result.
template <int K, int W, int KP>
__device__ __noinline__ float bank_dtw_ref(const float *xl, int L, const float *__restrict__ raw, float score_ref, float *Pb, int lane) {
    constexpr int B = 2 * W;
    float mu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = 0.f;
    for (int i = 0; i < L; ++i) {
#pragma unroll
        for (int k = 0; k < K; ++k) mu[k] += xl[i * KP + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = mu[k] / (float)L;
    for (int q = 0; q <= B; ++q) Pb[q * 64 + lane] = RP_INF;
    Pb[W * 64 + lane] = 0.f;
    for (int r = 1; r < L; ++r) {
        float left = RP_INF;
        for (int q = 0; q < B; ++q) {
            const int c = r - W + q;
            float v = RP_INF;
            if (c >= 1 && c <= L) {
                float dot_ab = 0.f, dot_a = 0.f, dot_b = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float ca = raw[(size_t)(r - 1) * K + k];
                    const float cb = xl[(c - 1) * KP + k] - mu[k];
                    dot_ab += ca * cb;   // -ffp-contract=off: a multiply and an add, as the reference
                    dot_a += ca * ca;
                    dot_b += cb * cb;
                }
                const float magnitude = sqrtf(dot_a * dot_b);
                const float sim = magnitude == 0.f ? 0.f : dot_ab / magnitude;
                v = (1.f - sim) + fminf(fminf(Pb[(q + 1) * 64 + lane], left), Pb[q * 64 + lane]);
            }
            Pb[q * 64 + lane] = v;
            left = v;
        }
    }
    return dtw_logistic(Pb[(W + 1) * 64 + lane] / (float)(L + L), score_ref);   // column n of row m-1 sits at band offset W + 1
}

}  // namespace rp
