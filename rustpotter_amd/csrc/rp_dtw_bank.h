// rp_dtw_bank.h -- the per-lane DTW walks of the wakeword-bank kernels, shared by rp_dtw_bank.hip (one wakeword per stream) and rp_dtw_set.hip
// (a set of wakewords per stream, alone or beside models): bank_dtw, bank_chk_window, bank_dtw_ref, and RP_BANK_LIVE_LANE, the lane of the
// three live kernels.  Device code only; include behind rp_device.h.
#pragma once
#include "rp_device.h"
#include "rp_dtw_lane.h"

namespace rp {

// One DTW of the lane's window against one template of L rows (m == n == L: the window is cut to the template's length keeping the oldest
// frames), built from the pieces the register kernels of rp_dtw.hip are built from (rp_dtw_lane.h): their column means, their ring column
// load, and dtw_band_wide_kernel's row sweep with one template -- two band cells per packed FMA, the template row a wave-uniform read
// (scalar loads), here as plain rows [L][K].  So a window gets the bits it gets from dtw_band_kernel / dtw_band2_kernel /
// dtw_band_wide_kernel (which differ in how many templates or windows share a packed instruction, not in a cell's operations) because it
// runs their code.  chk: the norm-range test of those kernels, same columns.
template <int K, int W, int KP>
__device__ __forceinline__ float bank_dtw(const float *xl, int L, const float *__restrict__ rows, float score_ref, float &chk_out) {
    constexpr int B = 2 * W;
    RP_DTW_COL_MEANS();   // mu
    RP_DTW_RING_START();  // ring, chk

    // P[q] = D[r-1][(r-1-W)+q]; row 0 has D[0][0] = 0 at q = W
    float P[B + 1];
#pragma unroll
    for (int q = 0; q <= B; ++q) P[q] = RP_INF;
    P[W] = 0.f;

#define RP_ROWS(GUARD) RP_DTW_ROW_BLOCK(RP_DTW_LOAD_COL, RP_DTW_WIDE_SWEEP(GUARD, rows + (size_t)(r - 1) * K, 1, P))
    {
        const int r0 = 1;
        RP_ROWS(true)
    }
    for (int r0 = 1 + B; r0 < L; r0 += B) { RP_ROWS(false) }
#undef RP_ROWS
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
// COPY: an out-of-line function with ONE calling kernel gets that kernel's LDS address of Pb as a constant; called from two kernels of one
// source it takes the address in a register and both kernels change.  Kernels that share a source and (K, W, KP) name a copy each.
template <int K, int W, int KP, int COPY = 0>
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

// The lane of the live kernels (dtw_bank_stream_kernel, dtw_set_stream_kernel, dtw_mixed_stream_kernel): row `row` of the call's flattened
// space is new window i of stream s for bank wakeword wi (live: wi lies inside the bank), and the window that ends at new frame i is lmax
// frames long -- the three kernels differ in how a row decodes to these and in where lmax comes from, nothing else.  The lane walks ITS
// wakeword, the averaged template first when it is to be scored, then the sample templates, so template count, template length and
// template rows are per-lane values: the template loop runs to the wave's largest count, bank_dtw's row loop to the wave's longest
// template, both under the lane mask, and template rows come by vector loads.  The gate is per lane: a window that did not pass leaves the
// walk, and the wave stops once no lane has a template left.  Norm-range test (dtw_bank_kernel recomputes for the whole wave once one lane
// is flagged: over fewer frames an unflagged lane stays unflagged), reference-shaped rescoring (the lanes that need it only) and the
// percentile block as dtw_bank_kernel; the cell arithmetic is bank_dtw's, so a stream gets the bits dtw_bank_kernel gives it.
// sl [kBankMaxTemplates][64]: a lane's scores (percentile modes), lane-minor; Pb [13][64]: band of the reference-shaped cell.  COPY: the
// kernel's copy of bank_dtw_ref (see there).  A macro, not a function: as a __forceinline__ function the same text compiled to other
// instruction streams in all 28 kernels (profiles/live_lane_fold.txt).
#define RP_BANK_LIVE_LANE(LMAX, COPY) \
    const BankWakeword *bw = bank_ww + (live ? wi : 0); \
    const float *xl = mfcc + (live ? ((size_t)s * q.frame_pitch + (q.first_new + i + 1 - (size_t)(LMAX))) * K : (size_t)0); \
    const float own_athr = bw->avg_threshold; \
    const float athr = own_athr == own_athr ? own_athr : q.avg_threshold; \
    const int avg_e = bw->avg, T = live ? bw->count : 0, first = bw->first, ref_only = bw->ref_only, window_chk = bw->window_chk; \
    const bool do_avg = live && avg_e >= 0 && athr != 0.f; \
    const int mode = q.score_mode; \
    float acc = 0.f, avg_sc = 0.f; \
    bool scored = live; \
    for (int ti = -1; __any(scored && ti < T); ++ti) { \
        const bool act = scored && ti < T && (ti >= 0 || do_avg); \
        float sc = 0.f, chk = 0.f; \
        int L = 1; \
        size_t off = 0; \
        if (act) { \
            const int e = ti < 0 ? avg_e : first + ti; \
            L = bank_tlen[e]; \
            off = (size_t)bank_trow[e] * K; \
            sc = bank_dtw<K, W, K>(xl, L, bank_unit + off, q.score_ref, chk); \
            if (window_chk && chk > kDtwFixLimit) chk = bank_chk_window<K, K>(xl, L); \
        } \
        const bool slow = act && (ref_only || chk > kDtwFixLimit); \
        const unsigned long long slow_mask = __ballot(slow); \
        if (slow_mask) { \
            if (slow) sc = bank_dtw_ref<K, W, K, COPY>(xl, L, bank_raw + off, q.score_ref, Pb, lane); \
            if (lane == 0 && fix) atomicAdd(dtw_fix_stats(fix), (unsigned long long)__popcll(slow_mask)); \
        } \
        if (act) { \
            if (ti < 0) { \
                avg_sc = sc; \
                if (q.gate && sc < athr) scored = false; \
            } else if (mode == 1) acc = ti == 0 ? sc : fmaxf(acc, sc); \
            else if (mode == 0) acc += sc; \
            else sl[ti * 64 + lane] = sc; \
        } \
    } \
    float a = 0.f; \
    if (scored) { \
        if (mode == 1) a = acc; \
        else if (mode == 0) a = acc / (float)T; \
        else { \
            for (int j = 1; j < T; ++j) { \
                const float x = sl[j * 64 + lane]; \
                int p = j - 1; \
                while (p >= 0 && sl[p * 64 + lane] > x) { sl[(p + 1) * 64 + lane] = sl[p * 64 + lane]; --p; } \
                sl[(p + 1) * 64 + lane] = x; \
            } \
            a = percentile_sorted(sl + lane, T, percentile_of_mode(mode), 64); \
        } \
    } \
    if (valid) { \
        agg[row] = a; \
        avg[row] = do_avg ? avg_sc : 0.f; \
    }

}  // namespace rp
