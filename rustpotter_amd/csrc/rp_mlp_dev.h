// rp_mlp_dev.h -- private to the wakeword-model kernels (rp_mlp.hip, rp_mlp_windows.hip, rp_mlp_stream.hip, rp_mlp_bank_stream.hip, rp_train_batch.hip): the
// operand splits, the tail layers, the window means' sums, pieces of the staged-frame kernels, and what mlp_route (rp_mlp.hip) needs from
// rp_mlp_windows.hip.  DESIGN.md §4.4.
#pragma once
#include "rp_device.h"

#include <algorithm>

namespace rp {

// ------------------------------------------------------------------ operand splits: eight floats -> the packed parts of one matrix operand
// f16 two-way split (kMlpF16x2): x0 = rtz_f16(x) (as f32: 13 mantissa bits cleared; below the f16 normal range the two differ
// by less than an f16 subnormal step, 6e-8), x1 = rtz_f16(x - x0).  rng: the largest |x| seen -- beyond the f16 range (features are MFCC
// coefficients, orders of magnitude below) a split would be silently wrong: such a row is listed and computed again with the f32 matrix
// instructions (one v_max_f32 |x| per feature finds it).
__device__ __forceinline__ void mlp_split_f16x2(const float (&xs)[8], u32x4 &p0, u32x4 &p1, float &rng) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = xs[2 * e], b = xs[2 * e + 1];
        rng = fmaxf(fmaxf(rng, fabsf(a)), fabsf(b));
        p0[e] = pkrtz(a, b);
        p1[e] = pk_f16_second(a - x0f(a), b - x0f(b));
    }
}

// three bf16 parts (kMlpBf16x3), exact: x0 = x & 0xffff0000 (a bf16), r = x - x0, x1 = r & 0xffff0000, x2 = r - x1 (at most 8 significant
// bits: a bf16 too); a packed register = the upper halves of two floats (v_perm).  bf16 has the f32 exponent range: nothing is listed.
__device__ __forceinline__ float mlp_bf16_rest(float x) { return x - __uint_as_float(__float_as_uint(x) & 0xffff0000u); }
__device__ __forceinline__ unsigned mlp_pk_bf16(float lo, float hi) { return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u); }
__device__ __forceinline__ void mlp_split_bf16x3(const float (&xs)[8], u32x4 &p0, u32x4 &p1, u32x4 &p2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = xs[2 * e], b = xs[2 * e + 1];
        const float ra = mlp_bf16_rest(a), rb = mlp_bf16_rest(b);
        p0[e] = mlp_pk_bf16(a, b);
        p1[e] = mlp_pk_bf16(ra, rb);
        p2[e] = mlp_pk_bf16(mlp_bf16_rest(ra), mlp_bf16_rest(rb));
    }
}

// ------------------------------------------------------------------ tail layers of one row (mlp_mfma_kernel and the staged-frame kernels)
// Lane = (row, output phase ph of NPH): outputs strided by NPH over the phases.  tl: the tail weights (W_l [out][in] then b_l [out], layer
// after layer), d1 .. d4 the layer widths behind layer 1; hin: the row's layer-1 outputs, h2: the row's hidden layer, both read and
// written through at(i) (plain, or rotated by the row against bank conflicts); sync(): the hidden layer is complete before anyone reads it.
// Even inputs accumulate in s0, odd ones in s1, (s0 + s1) + bias: the order every kernel of the forward shares.
template <int NPH, class At, class Sync>
__device__ __forceinline__ void mlp_tail_layers(const float *tl, int n_layers, int d1, int d2, int d3, int d4, const float *hin, float *h2, int ph,
                                                bool row_ok, float *dst, At at, Sync sync) {
    const int dd[4] = {d1, d2, d3, d4};
    const float *wp = tl;
    int cur_in = d1;
    if (n_layers == 1 && row_ok)
        for (int o = ph; o < d1; o += NPH) dst[o] = hin[at(o)];
    for (int layer = 1; layer < n_layers; ++layer) {
        const int on = dd[layer];
        const bool last = layer + 1 == n_layers;
        for (int o = ph; o < on; o += NPH) {
            const float *wr = wp + (size_t)o * cur_in;
            float s0 = 0.f, s1 = 0.f;
            int i = 0;
            for (; i + 1 < cur_in; i += 2) { s0 = fmaf(hin[at(i)], wr[i], s0); s1 = fmaf(hin[at(i + 1)], wr[i + 1], s1); }
            if (i < cur_in) s0 = fmaf(hin[at(i)], wr[i], s0);
            float sacc = (s0 + s1) + wp[(size_t)on * cur_in + o];
            if (!last && sacc < 0.f) sacc = 0.f;
            if (last) { if (row_ok) dst[o] = sacc; } else h2[at(o)] = sacc;
        }
        sync();
        wp += (size_t)on * cur_in + on;
        cur_in = on;
        hin = h2;
    }
}

// ------------------------------------------------------------------ window means (rp_mlp_windows.hip, rp_mlp_bank_stream.hip)
// per window the column means over its L frames, summed in frame order like MfccNormalizer::normalize
// (src/mfcc/normalizer.rs:3-31); one lane per (window, four coefficients), nw <= 64 consecutive windows of a stream per block: frames
// src[0 .. nw + L - 1) of K coefficients -> dst [nw][K]
__device__ __forceinline__ void window_means_body(const float *__restrict__ src, int nw, int L, int K, float *__restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *fs = reinterpret_cast<float *>(smem);  // [64 + L - 1][K]
    const int nfr = nw + L - 1;
    // (eight loads in flight per wait in both loops; the kernel is bound by the LDS reads of the sums -- 64 x K x L per block, each
    // window summed in frame order as MfccNormalizer::normalize does -- 0.22 ms for 4 096 streams x 202 windows either way)
#pragma unroll 8
    for (int i = threadIdx.x; i < nfr * K; i += 256) fs[i] = src[i];
    __syncthreads();
    // four coefficients per lane (K % 4 == 0, launch_window_means): 16-byte LDS reads move twice the bytes per LDS cycle of 4-byte ones
    // and a lane's four sums are independent chains (round 4: 1.81 -> 1.02 ms for 32 768 streams x 202 windows)
    const int K4 = K / 4;
    for (int i = threadIdx.x; i < nw * K4; i += 256) {
        const int w = i / K4, q = i - w * K4;
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        const float *col = fs + w * K + 4 * q;
#pragma unroll 8
        for (int f = 0; f < L; ++f) sum += *reinterpret_cast<const f32x4 *>(col + f * K);   // sequential sums, as MfccNormalizer::normalize
        const float n = (float)L;
        *reinterpret_cast<f32x4 *>(dst + (size_t)w * K + 4 * q) = f32x4{sum.x / n, sum.y / n, sum.z / n, sum.w / n};
    }
}

// ------------------------------------------------------------------ the staged-frame kernels (rp_mlp_windows.hip)
constexpr int kWinWaves = 4, kWinTile = 32, kWinMaxTiles = 7, kWinAhead = 3;

// The cut of a stream's n_win windows into workgroups, the one rule of mlp_route (host) and mlp_windows_bank_kernel (device, per stream): as
// few workgroups per stream as `cap` <= 7 tiles of 32 windows each allow, the tiles spread evenly over them.  A window's bits depend on
// this cut (BITS, rp_mlp_windows.hip), so it exists once.
struct WinCut { int tiles; unsigned bps; };   // tiles per workgroup, workgroups per stream
__host__ __device__ inline WinCut mlp_windows_cut(size_t n_win, int cap = kWinMaxTiles) {
    const size_t tiles = (n_win + kWinTile - 1) / kWinTile;
    if (tiles == 0) return WinCut{0, 0u};
    const size_t wgs = (tiles + cap - 1) / cap, per = (tiles + wgs - 1) / wgs;
    return WinCut{(int)per, (unsigned)((n_win + per * kWinTile - 1) / (per * kWinTile))};
}
// frame slots of a workgroup of `tiles` tiles over windows of L frames
__host__ __device__ inline int mlp_windows_slots(int tiles, int L) { return (tiles * kWinTile + L + 3) & ~3; }
// LDS bytes of a workgroup: tail weights, a flag per frame slot, the frame planes (`parts` parts x two k-halves) -- later the sums of
// `tiles` tiles (h1 of a tile in its place) + h2 of the four waves, or in the wide form (nq > 0 output tiles) h1 [32][32 nq + 1] + h2 [32][33]
inline size_t mlp_windows_lds(int tail_floats, int slots, int tiles, int parts, int nq) {
    const size_t later = nq == 0 ? (size_t)tiles * 4096 + (size_t)kWinWaves * 4096 : (size_t)32 * (32 * nq + 1) * 4 + (size_t)32 * 33 * 4;
    return (size_t)((tail_floats + 3) & ~3) * 4 + (size_t)slots * 4 + std::max((size_t)2 * parts * slots * 16, later);
}

// What mlp_route decides for the staged-frame kernels: 32-window row tiles per workgroup (NT), 32-output tiles (NQ, the wide form), frame
// slots, workgroups per stream, LDS bytes
struct WinRoute {
    int tiles = 0, nq = 0, slots = 0;
    size_t bps = 0, lds = 0;
};
// mlp_windows_kernel / mlp_windows_wide_kernel over the q.S streams of q; p3: three bf16 parts, else two f16 parts (rows listed in redo)
hipError_t launch_mlp_windows(hipStream_t st, const MlpDev &m, const WinRoute &r, const MlpForward &q, bool p3, uint32_t *redo);
hipError_t launch_mlp_windows_wide(hipStream_t st, const MlpDev &m, const WinRoute &r, const MlpForward &q, bool p3, uint32_t *redo);

// ---- frames [fb, fe) of the windows, one 32-output tile, up to NT row tiles: window row w at k-step f is slot w + f of the planes A.  The
// weight fragments come straight from the lane-ordered image wimg [frame][NQ output tiles][part][k-half][output] into registers, kWinAhead
// frames ahead; q: the wave's output tile (NQ = 1, q = 0 in the narrow form).  nt_here <= NT: the tiles that exist (a constant NT folds
// every test on it away); tiles behind it are skipped, wave-uniformly.
//  !P3: x0 w0 + x1 w0 + x0 w1 on v_mfma_f32_32x32x16_f16.  P3: six v_mfma_f32_32x32x16_bf16 per tile (x_i w_j, i + j <= 2, smallest first).
// mlp_windows_wide_kernel keeps its own copy of this loop, of the staging and of the tail: through these helpers its three-part form
// measured 1 % slower (Large model, 32 768 streams: forward 109.7 -> 110.4 ms with this sweep alone, 111.0 with the other helpers alone).
template <int NT, bool P3, int NQ>
__device__ __forceinline__ void mlp_windows_sweep(const u32x4 *A, int slots, int fb, int fe, const u32x4 *__restrict__ wimg, int q,
                                                  int nt_here, v16f (&acc)[NT]) {
    constexpr int NPART = P3 ? 3 : 2;
    const int l = threadIdx.x & 63, lr = l & 31, lh = l >> 5;
    u32x4 wq0[kWinAhead], wq1[kWinAhead], wq2[P3 ? kWinAhead : 1];   // the weight fragments of the next kWinAhead frames, 16 bytes each
    auto wfetch = [&](int f, int j) __attribute__((always_inline)) {
        const int fc = f < fe ? f : fe - 1;
        wq0[j] = wimg[((((size_t)fc * NQ + q) * NPART + 0) * 2 + lh) * 32 + lr];
        wq1[j] = wimg[((((size_t)fc * NQ + q) * NPART + 1) * 2 + lh) * 32 + lr];
        if (P3) wq2[j] = wimg[((((size_t)fc * NQ + q) * NPART + 2) * 2 + lh) * 32 + lr];
    };
    if (fb >= fe) return;
#pragma unroll
    for (int j = 0; j < kWinAhead; ++j) wfetch(fb + j, j);
    const u32x4 *A0 = A + (0 * 2 + lh) * slots + lr, *A1 = A + (1 * 2 + lh) * slots + lr;
    const u32x4 *A2 = A + ((P3 ? 2 : 0) * 2 + lh) * slots + lr;
    (void)A2;
    for (int f0 = fb; f0 < fe; f0 += kWinAhead) {
#pragma unroll
        for (int j = 0; j < kWinAhead; ++j) {
            const int f = f0 + j;
            if (f < fe) {   // wave-uniform
                if (P3) {   // six products per tile, smallest first; tiles in pairs so that consecutive matrix instructions do not wait on each other
                    const bf16x8 c0 = __builtin_bit_cast(bf16x8, wq0[j]), c1 = __builtin_bit_cast(bf16x8, wq1[j]), c2 = __builtin_bit_cast(bf16x8, wq2[j]);
                    wfetch(f + kWinAhead, j);
#pragma unroll
                    for (int t = 0; t < NT; t += 2) {
                        if (t >= nt_here) break;   // wave-uniform
                        const bool two = t + 1 < NT && t + 1 < nt_here;
                        const bf16x8 x0 = __builtin_bit_cast(bf16x8, A0[t * kWinTile + f]), x1 = __builtin_bit_cast(bf16x8, A1[t * kWinTile + f]),
                                     x2 = __builtin_bit_cast(bf16x8, A2[t * kWinTile + f]);
                        bf16x8 y0 = x0, y1 = x1, y2 = x2;
                        if (two) {
                            y0 = __builtin_bit_cast(bf16x8, A0[(t + 1) * kWinTile + f]); y1 = __builtin_bit_cast(bf16x8, A1[(t + 1) * kWinTile + f]);
                            y2 = __builtin_bit_cast(bf16x8, A2[(t + 1) * kWinTile + f]);
                        }
#define RP_WIN6(XA, XB, WB)                                                                                        \
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(XA, WB, acc[t], 0, 0, 0);                 \
                        if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(XB, WB, acc[t + 1], 0, 0, 0);
                        RP_WIN6(x0, y0, c2) RP_WIN6(x1, y1, c1) RP_WIN6(x2, y2, c0) RP_WIN6(x0, y0, c1) RP_WIN6(x1, y1, c0) RP_WIN6(x0, y0, c0)
#undef RP_WIN6
                    }
                    continue;
                }
                const f16x8 b0 = __builtin_bit_cast(f16x8, wq0[j]), b1v = __builtin_bit_cast(f16x8, wq1[j]);
                wfetch(f + kWinAhead, j);
                // tiles in pairs: the two parts of two tiles live at a time (all NT at once cost 8 NT registers and the third wave
                // per SIMD), and the three products of a tile are one other matrix instruction apart
#pragma unroll
                for (int t = 0; t < NT; t += 2) {
                    if (t >= nt_here) break;   // wave-uniform
                    const bool two = t + 1 < NT && t + 1 < nt_here;
                    const f16x8 p0 = __builtin_bit_cast(f16x8, A0[t * kWinTile + f]), p1 = __builtin_bit_cast(f16x8, A1[t * kWinTile + f]);
                    f16x8 q0 = p0, q1 = p1;
                    if (two) { q0 = __builtin_bit_cast(f16x8, A0[(t + 1) * kWinTile + f]); q1 = __builtin_bit_cast(f16x8, A1[(t + 1) * kWinTile + f]); }
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p0, b0, acc[t], 0, 0, 0);
                    if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(q0, b0, acc[t + 1], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p1, b0, acc[t], 0, 0, 0);
                    if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(q1, b0, acc[t + 1], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p0, b1v, acc[t], 0, 0, 0);
                    if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(q0, b1v, acc[t + 1], 0, 0, 0);
                }
            }
        }
    }
}

// ---- layer-1 value of a window row: the sum over the staged frames (taken relative to c), the rest of the row's own mean mu taken out
// through the weight sums ws of this output (W.(f - mu) = W.(f - c) - sum_k (mu - c)[k] wsum[k]), bias, ReLU
__device__ __forceinline__ float mlp_windows_layer1(float sum, const float4 *mu, const float4 (&c4)[4], const float4 (&ws4)[4], float bias1, bool relu1) {
    float corr = 0.f;   // - sum_k (mu[row][k] - c[k]) * wsum[o][k]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 m4 = mu[k], w4 = ws4[k], c = c4[k];
        corr = fmaf(m4.x - c.x, w4.x, corr); corr = fmaf(m4.y - c.y, w4.y, corr); corr = fmaf(m4.z - c.z, w4.z, corr); corr = fmaf(m4.w - c.w, w4.w, corr);
    }
    float v = sum - corr;
    v += bias1;
    if (relu1 && v < 0.f) v = 0.f;
    return v;
}

// ---- one row of the trainer's loss (train_softmax_grad_kernel in rp_mlp.hip, train_batch_kernel in rp_train_batch.hip): log_softmax
// (x - max - ln(sum exp(x - max))), loss_row = -log_sm[label], dlogits = (softmax - onehot) / B
__device__ __forceinline__ void train_softmax_row(const float *x, int lab, size_t B, int C, float *dz, float *loss_row) {
    float mx = x[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
    const float lse = logf(se);
    for (int c = 0; c < C; ++c) {
        const float lsm = (x[c] - mx) - lse;
        if (c == lab) *loss_row = -lsm;
        dz[c] = (expf(lsm) - (c == lab ? 1.f : 0.f)) / (float)B;
    }
}

// ------------------------------------------------------------------ a window's decision (rp_mlp.hip, rp_mlp_model_set.hip)
// calc_inverse_similarity, wakeword_nn.rs:161-163
__device__ __forceinline__ float nn_inverse_similarity(float n1, float n2, float reference) {
    return 1.f - (1.f / (1.f + expf(((n1 - n2) - reference) / reference)));
}

// the integer f32::total_cmp orders by: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
__device__ __forceinline__ int nn_total_cmp_key(float x) {
    const int b = __float_as_int(x);
    return b ^ (int)((unsigned)(b >> 31) >> 1);
}

// get_label (:47-60: max_by(total_cmp) keeps the LAST maximum), run_detection_by_label (:61-99: second_prob is the
// smallest other logit), validate_scores (:113-123)
// one window's logits lg [nl] -> its label, score (-2: no valid detection) and avg score
// A NaN logit is ordered as total_cmp orders it: a positive NaN is the maximum and stays the label, its scores are NaN and fail both
// gates (>= is false), so the window never passes -- unless that label is the none label, which is no detection either; a negative NaN is
// the smallest value.  second_prob leaves out only what == the label's value (nothing, when that is NaN) and is the total_cmp minimum
// of the rest.  The rp_detector.cpp loop and the oracle's follow the same rule.
__device__ __forceinline__ void nn_score_row(const float *__restrict__ lg, int nl, int none_index, float ref, int calc_avg, float threshold,
                                             float avg_threshold, float *score_out, float *avg_out, int *label_out) {
    int bi = 0;
    for (int i = 1; i < nl; ++i) if (!(nn_total_cmp_key(lg[i]) < nn_total_cmp_key(lg[bi]))) bi = i;
    float score = -2.f, av = 0.f;
    if (bi != none_index) {
        const float label_prob = lg[bi], none_prob = none_index >= 0 ? lg[none_index] : 0.f;
        float second = 0.f;
        if (calc_avg) {
            bool any = false;
            for (int i = 0; i < nl; ++i) {
                if (lg[i] == label_prob) continue;
                if (!any || !(nn_total_cmp_key(lg[i]) > nn_total_cmp_key(second))) { second = lg[i]; any = true; }
            }
            if (!any) second = 0.f;
            av = nn_inverse_similarity(label_prob, second, ref);
        }
        const float sc = nn_inverse_similarity(label_prob, none_prob, ref);
        if (sc >= threshold && av >= avg_threshold) score = sc;
    }
    *score_out = score; *avg_out = av; *label_out = bi;
}

}  // namespace rp
