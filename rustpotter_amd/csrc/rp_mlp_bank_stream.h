// rp_mlp_bank_stream.h -- the body of the live forwards over a model bank: mlp_bank_stream_kernel (rp_mlp_bank_stream.hip, a model per stream)
// and mlp_set_stream_kernel (rp_mlp_model_set.hip, a set of models per stream) are thin fronts of mlp_bank_stream_body.  ARITHMETIC, WEIGHTS
// and SHAPE are written up in rp_mlp_bank_stream.hip.  Device code only.
#pragma once
#include "rp_mlp_dev.h"

namespace rp {

constexpr int kBsAhead = 2;     // k-blocks whose loads are in flight ahead of the matrix instructions
constexpr int kBsH1 = 33;       // floats per row of h1 / h2 in LDS (32 outputs + 1 against bank conflicts)

// One wave: up to RT tiles of 16 of the n_new windows of one stream, rows r0 .. of them, with the model of bank entry e.  x0: the frame the
// stream's first window of the call starts at (window `row` starts `row` frames behind it and reads e.L frames); mean_s [n_new][16] and out_s
// [n_new][label_pitch]: the rows of the same windows.  h1 / h2: [16][kBsH1] floats of LDS each.
template <int RT>
__device__ __forceinline__ void mlp_bank_stream_body(const ModelBankDev &bank, const ModelBankEntry &e, const float *__restrict__ x0,
                                                     const float *__restrict__ mean_s, float *__restrict__ out_s, int n_new, int r0, float *h1,
                                                     float *h2) {
    const int l = threadIdx.x, li = l & 15, lk = l >> 4;
    const int rows_here = n_new - r0 < 16 * RT ? n_new - r0 : 16 * RT;
    const int label_pitch = bank.label_pitch;
    float *orow = out_s + (size_t)r0 * (size_t)label_pitch;
    const int L = e.L;
    const int nblk = (16 * L + 127) / 128 * 4;   // kpad / 32
    const bool two = e.n1p > 16;
    const int tiles_here = (rows_here + 15) / 16;
    const u32x4 *__restrict__ wimg = static_cast<const u32x4 *>(bank.wimg) + e.wimg + (lk & 1) * 32 + li;
    const float *xr[RT];
    float4 mu_a[RT], mu_b[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        int row = r0 + 16 * t + li;
        if (row >= n_new) row = n_new - 1;   // rows past the end recompute the last row; their results are dropped
        xr[t] = x0 + (size_t)row * 16 + 8 * (lk & 1);
        // mfcc_size 16: a lane's pieces always hold coefficients 8 (lk & 1) .. + 8
        const float4 *mu = reinterpret_cast<const float4 *>(mean_s + (size_t)row * 16);
        mu_a[t] = mu[2 * (lk & 1)]; mu_b[t] = mu[2 * (lk & 1) + 1];
    }
    f32x4 acc[RT][2];
#pragma unroll
    for (int t = 0; t < RT; ++t) { acc[t][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[t][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    // block u: this lane's k = 32 u + 8 lk .. + 8 lie in frame f = 2 u + (lk >> 1), half lk & 1
    u32x4 bq[kBsAhead][2][3];
    float4 aq[kBsAhead][RT][2];
#pragma unroll
    for (int j = 0; j < kBsAhead; ++j) {
#pragma unroll
        for (int p = 0; p < 3; ++p) { bq[j][0][p] = (u32x4){0u, 0u, 0u, 0u}; bq[j][1][p] = (u32x4){0u, 0u, 0u, 0u}; }
#pragma unroll
        for (int t = 0; t < RT; ++t) { aq[j][t][0] = make_float4(0.f, 0.f, 0.f, 0.f); aq[j][t][1] = make_float4(0.f, 0.f, 0.f, 0.f); }
    }
    auto fetch = [&](int u, int j) __attribute__((always_inline)) {
        const int f = 2 * u + (lk >> 1), fc = f < L ? f : L - 1;   // a lane past the window loads its last frame and takes zeros instead
        const u32x4 *wp = wimg + (size_t)fc * 192;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            bq[j][0][p] = wp[p * 64];
            if (two) bq[j][1][p] = wp[p * 64 + 16];   // wave-uniform
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
            if (t < tiles_here) {   // wave-uniform
                aq[j][t][0] = *reinterpret_cast<const float4 *>(xr[t] + (size_t)fc * 16);
                aq[j][t][1] = *reinterpret_cast<const float4 *>(xr[t] + (size_t)fc * 16 + 4);
            }
    };
#pragma unroll
    for (int j = 0; j < kBsAhead; ++j)
        if (j < nblk) fetch(j, j);
    for (int u0 = 0; u0 < nblk; u0 += kBsAhead) {
#pragma unroll
        for (int j = 0; j < kBsAhead; ++j) {
            const int u = u0 + j;
            if (u >= nblk) continue;   // wave-uniform
            const bool ok = 2 * u + (lk >> 1) < L;
            bf16x8 c[2][3];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int p = 0; p < 3; ++p) c[n][p] = __builtin_bit_cast(bf16x8, ok ? bq[j][n][p] : (u32x4){0u, 0u, 0u, 0u});
            float4 lo[RT], hi[RT];
#pragma unroll
            for (int t = 0; t < RT; ++t) { lo[t] = aq[j][t][0]; hi[t] = aq[j][t][1]; }
            if (u + kBsAhead < nblk) fetch(u + kBsAhead, j);
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                if (t >= tiles_here) continue;   // wave-uniform
                const float4 ma = mu_a[t], mb = mu_b[t];
                float xs[8] = {lo[t].x - ma.x, lo[t].y - ma.y, lo[t].z - ma.z, lo[t].w - ma.w, hi[t].x - mb.x, hi[t].y - mb.y, hi[t].z - mb.z, hi[t].w - mb.w};
                if (!ok) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) xs[i] = 0.f;
                }
                u32x4 p0, p1, p2;
                mlp_split_bf16x3(xs, p0, p1, p2);
                const bf16x8 av0 = __builtin_bit_cast(bf16x8, p0), av1 = __builtin_bit_cast(bf16x8, p1), av2 = __builtin_bit_cast(bf16x8, p2);
#define RP_BS6(XA, P)                                                                                              \
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(XA, c[0][P], acc[t][0], 0, 0, 0);              \
                if (two) acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(XA, c[1][P], acc[t][1], 0, 0, 0);
                RP_BS6(av0, 2) RP_BS6(av1, 1) RP_BS6(av2, 0) RP_BS6(av0, 1) RP_BS6(av1, 0) RP_BS6(av0, 0)
#undef RP_BS6
            }
        }
    }
    // ---- layer-1 bias (+ReLU) -> LDS, C/D layout: col = lane & 15, row = (lane >> 4) * 4 + reg; then the tail layers, tile by tile
    const float *__restrict__ b1 = bank.b1 + e.b1;
    const float *__restrict__ tl = bank.tail + e.tail;
    const bool relu1 = e.n_layers > 1;
    const int rr = l & 15, ph = l >> 4;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        if (t >= tiles_here) continue;   // wave-uniform
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (n == 1 && !two) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = acc[t][n][q];
                v += b1[16 * n + li];
                if (relu1 && v < 0.f) v = 0.f;
                h1[(4 * lk + q) * kBsH1 + 16 * n + li] = v;
            }
        }
        wave_lds_sync();
        const bool row_ok = 16 * t + rr < rows_here;
        float *dst = orow + (size_t)(row_ok ? 16 * t + rr : 0) * (size_t)label_pitch;
        mlp_tail_layers<4>(tl, e.n_layers, e.d1, e.d2, e.d3, 0, h1 + rr * kBsH1, h2 + rr * kBsH1, ph, row_ok, dst, [](int i) { return i; },
                           [] { wave_lds_sync(); });
        if (row_ok && ph == 0)
            for (int o = e.n_labels; o < label_pitch; ++o) dst[o] = 0.f;   // behind the model's labels
        wave_lds_sync();   // h1 / h2 are free for the next tile
    }
}

}  // namespace rp
