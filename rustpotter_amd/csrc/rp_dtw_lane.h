// rp_dtw_lane.h -- the per-lane walk of the register DTW kernels, each piece once: dtw_band_kernel / dtw_band2_kernel / dtw_band_wide_kernel
// (rp_dtw.hip) and bank_dtw (rp_dtw_bank.h) are built from it and keep only what is their own.  Device code only; include behind rp_device.h.
//
// The kernels sit on the register cliff (256 registers, one or two waves per SIMD at band 5 / 6), and the compiler's scheduling and register
// allocation follow the shape of the source: as __forceinline__ functions the column means, the lane maps and the score epilogue each moved
// instructions in every build that used them, and a one-trip template loop around the sweep moved the norm-range maximum inside the hot
// loop of every bank kernel (profiles/register_dtw_lane.txt).  So the pieces are MACROS, expanded where the copies used to stand: textually
// the program the kernels were before, and the same instruction streams.  A macro's comment names the variables it takes from the kernel's
// scope.  A piece becomes a function only with timings that show the moved code costs nothing.
#pragma once
#include "rp_device.h"

namespace rp {

constexpr int kDtwWin = 64;   // lanes of a wave: windows per wave (dtw_band2_kernel: two per lane)

// ---- lane -> window, frames from global memory -------------------------------------------------------------------------------------------
// A wave's lanes are consecutive entries of the flattened (stream, window) space, or of the gate's list (GateList::list: row ids
// s * n_win + w of the windows that passed gate_compact_kernel; the grid is sized for every window, tiles past the list's end have nothing
// to do).  NW entries per tile: 64, or 128 with two windows per lane.
// Entry F of the launch, in a tile of NW entries -> stream, window, valid, the first frame of the window in memory (pitch K).  The wave
// leaves at once in a list-mode tile past the end of the list or behind a dense list, and in a DENSE-mode launch (no list, a count) whose
// list is not dense.  A lane past the end walks the last listed window (the first window of the call) and stores nothing.  Takes gl, tile,
// n_streams, n_win, mfcc, frame_pitch, first_win and K from the scope.
#define RP_DTW_GLOBAL_ENTRY(NW, F, s_, w_, valid_, xl_)                                                \
    do {                                                                                               \
        size_t f_ = (F);                                                                               \
        if (gl.list) {                                                                                 \
            const uint32_t n_listed = *gl.count;                                                       \
            if ((size_t)tile * (NW) >= n_listed || (gl.dense_min && n_listed >= gl.dense_min)) return; \
            valid_ = f_ < n_listed;                                                                    \
            f_ = gl.list[(valid_) ? f_ : n_listed - 1];                                                \
        } else {                                                                                       \
            if (gl.count && *gl.count < gl.dense_min) return;                                          \
            valid_ = f_ < n_streams * n_win;                                                           \
        }                                                                                              \
        s_ = (valid_) ? f_ / n_win : 0;                                                                \
        w_ = (valid_) ? f_ - s_ * n_win : 0; /* an int or a size_t */                                  \
        xl_ = mfcc + (s_ * frame_pitch + first_win + (size_t)w_) * K;                                  \
    } while (0)

// ---- lane -> window, frames staged in LDS ------------------------------------------------------------------------------------------------
// A tile of NW windows is up to two stream segments A and B of n + L + W frames each, staged at pitch KP.  flat != 0: the tile is NW
// consecutive entries of the flattened (stream, window) space, so a wave may straddle two streams (needs n_win >= NW) and no lane is wasted
// on a ragged last tile (`tiles` then counts flattened tiles and there is no stream index); flat == 0: tiles never cross a stream.
// Declares sA, sB, wA, nA, nB, segA; takes tile, lane, L, xs, mfcc, frame_pitch, n_frames_total, first_win, n_win, n_streams, tiles,
// n_chunks, flat and K, KP, W from the kernel.  Ends with the barrier.
#define RP_DTW_STAGE_SEGMENTS(NW)                                                                      \
    size_t sA, sB = 0;                                                                                 \
    int wA, nA, nB = 0;                                                                                \
    if (flat) {                                                                                        \
        const size_t f0 = (size_t)tile * (NW);                                                         \
        sA = f0 / n_win;                                                                               \
        wA = (int)(f0 - sA * n_win);                                                                   \
        nA = (int)n_win - wA < (NW) ? (int)n_win - wA : (NW);                                          \
        if (nA < (NW) && sA + 1 < n_streams) { sB = sA + 1; nB = (NW) - nA; }                          \
    } else {                                                                                           \
        sA = blockIdx.x / ((size_t)tiles * n_chunks);                                                  \
        wA = (int)tile * (NW);                                                                         \
        nA = (int)n_win - wA < (NW) ? (int)n_win - wA : (NW);                                          \
    }                                                                                                  \
    const int segA = nA + L + W; /* frames staged for the first stream segment */                      \
    {                                                                                                  \
        const float *src = mfcc + sA * frame_pitch * K;                                                \
        const size_t g0 = first_win + wA;                                                              \
        for (int i = lane; i < segA * K; i += kDtwWin) {                                               \
            int f = i / K, k = i - f * K;                                                              \
            size_t g = g0 + f;                                                                         \
            xs[f * KP + k] = g < n_frames_total ? src[g * K + k] : 0.f;                                \
        }                                                                                              \
    }                                                                                                  \
    if (nB > 0) {                                                                                      \
        const float *src = mfcc + sB * frame_pitch * K;                                                \
        const int segB = nB + L + W;                                                                   \
        for (int i = lane; i < segB * K; i += kDtwWin) {                                               \
            int f = i / K, k = i - f * K;                                                              \
            size_t g = first_win + f;                                                                  \
            xs[(segA + f) * KP + k] = g < n_frames_total ? src[g * K + k] : 0.f;                       \
        }                                                                                              \
    }                                                                                                  \
    __syncthreads()
// entry `ent` (0 .. NW - 1) of the staged tile -> stream, window, valid, the first frame of the window in LDS
#define RP_DTW_STAGED_ENTRY(ent, s_, w_, valid_, xl_)                                                  \
    do {                                                                                               \
        const bool inA = (ent) < nA;                                                                   \
        valid_ = inA || ((ent) - nA < nB);                                                             \
        s_ = inA ? sA : sB;                                                                            \
        w_ = inA ? wA + (ent) : (ent) - nA;                                                            \
        xl_ = xs + (inA ? (ent) : ((valid_) ? segA + (ent) - nA : 0)) * KP;                            \
    } while (0)

// ---- column means --------------------------------------------------------------------------------------------------------------------------
// MfccNormalizer::normalize, src/mfcc/normalizer.rs:17-29: sequential column sums over the window's L frames, / L.  dtw_mean_unroll(K)
// frames are in flight per wait (left rolled, every frame of a window paid a whole LDS / memory round trip): 10 at mfcc_size 5; 13 / 16
// components per frame keep the register count where it was with four.  -DRP_DTW_MEAN_UNROLL= / -DRP_DTW_MEAN_UNROLL_WIDE= override them.
#ifndef RP_DTW_MEAN_UNROLL
#define RP_DTW_MEAN_UNROLL 10
#endif
#ifndef RP_DTW_MEAN_UNROLL_WIDE
#define RP_DTW_MEAN_UNROLL_WIDE 4
#endif
constexpr int dtw_mean_unroll(int K) { return K <= 5 ? RP_DTW_MEAN_UNROLL : RP_DTW_MEAN_UNROLL_WIDE; }

// Declares float mu[K]; takes xl, L and K, KP from the scope.
#define RP_DTW_COL_MEANS()                                                                \
    float mu[K];                                                                          \
    _Pragma("unroll") for (int k = 0; k < K; ++k) mu[k] = 0.f;                            \
    _Pragma("unroll dtw_mean_unroll(K)") for (int i = 0; i < L; ++i) {                    \
        _Pragma("unroll") for (int k = 0; k < K; ++k) mu[k] += xl[i * KP + k];            \
    }                                                                                     \
    _Pragma("unroll") for (int k = 0; k < K; ++k) mu[k] = mu[k] / (float)L
// Two windows at once, (window x0, window x1) per component: declares v2f mu[K]; takes x0, x1, L and K, KP from the scope.
#define RP_DTW_COL_MEANS2()                                                                                   \
    v2f mu[K];                                                                                                \
    _Pragma("unroll") for (int k = 0; k < K; ++k) mu[k] = (v2f){0.f, 0.f};                                    \
    _Pragma("unroll dtw_mean_unroll(K)") for (int i = 0; i < L; ++i) {                                        \
        _Pragma("unroll") for (int k = 0; k < K; ++k) mu[k] += (v2f){x0[i * KP + k], x1[i * KP + k]};         \
    }                                                                                                         \
    const float fl = (float)L;                                                                                \
    _Pragma("unroll") for (int k = 0; k < K; ++k) mu[k] = (v2f){mu[k].x / fl, mu[k].y / fl}

// ---- ring column load ------------------------------------------------------------------------------------------------------------------------
// Column c of the window (frame c - 1), mean taken out, scaled to unit length by rsqrtf of the fma-chained squared norm (a zero vector stays
// zero), into ring slot `slot` (a compile-time value wherever it is used): ring[j][k] = { y_slot(2j)[k], y_slot(2j+1)[k] }.
// chk: max over the frames loaded of (squared norm, its reciprocal square root), one v_max3_f32 -- the norm-range test: > kDtwFixLimit ->
// the window is listed for dtw_ref_kernel.  Takes xl, mu, ring, chk and K, KP from the scope.
#define RP_DTW_LOAD_COL(c, slot)                                                          \
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
// The start of a walk: declares the ring (zero) and chk, and loads columns 1 .. W - 1, the part of row 1's band that lies inside the window.
// Takes what RP_DTW_LOAD_COL takes, and B, W.
#define RP_DTW_RING_START()                                                               \
    v2f ring[B / 2][K];                                                                   \
    _Pragma("unroll") for (int j = 0; j < B / 2; ++j)                                     \
        _Pragma("unroll") for (int k = 0; k < K; ++k) ring[j][k] = (v2f){0.f, 0.f};       \
    float chk = 0.f;                                                                      \
    _Pragma("unroll") for (int c = 1; c < W; ++c) RP_DTW_LOAD_COL(c, c % B)
// The two-window twin: ring[slot][k] = the slot's unit-length frame of (window x0, window x1), chk the pair of norm-range tests.  Takes x0,
// x1, mu, ring, chk and K, KP from the scope.
#define RP_DTW_LOAD_COL2(c, slot)                                                                   \
    do {                                                                                            \
        v2f y_[K], bb_ = (v2f){0.f, 0.f};                                                           \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                             \
            y_[k] = (v2f){x0[((c)-1) * KP + k], x1[((c)-1) * KP + k]} - mu[k];                      \
            bb_ = __builtin_elementwise_fma(y_[k], y_[k], bb_);                                     \
        }                                                                                           \
        const v2f inv_ = (v2f){bb_.x > 0.f ? rsqrtf(bb_.x) : 0.f, bb_.y > 0.f ? rsqrtf(bb_.y) : 0.f}; \
        chk.x = fmaxf(fmaxf(chk.x, inv_.x), bb_.x); chk.y = fmaxf(fmaxf(chk.y, inv_.y), bb_.y);     \
        _Pragma("unroll") for (int k = 0; k < K; ++k) ring[slot][k] = y_[k] * inv_;                 \
    } while (0)

// ---- a block of 2W rows ------------------------------------------------------------------------------------------------------------------
// Rows r0 .. r0 + 2W - 1, cut by r < L (rows 1..m-1 only: row m is never read, dtw.rs:101), unrolled so that every ring slot and band index
// is a compile-time register: LOAD_COL (RP_DTW_LOAD_COL or its twin) brings column r + W - 1 of the window into the ring, then the kernel's
// row body runs with u and r in scope.  Takes r0, L and W, B from the scope.
#define RP_DTW_ROW_BLOCK(LOAD_COL, ...)                                                                \
    _Pragma("unroll") for (int u = 0; u < B; ++u) {                                                    \
        const int r = r0 + u;                                                                          \
        if (r < L) {                                                                                   \
            LOAD_COL(r + W - 1, (u + W) % B);                                                          \
            __VA_ARGS__                                                                                \
        }                                                                                              \
    }

// The serial min chain of a row whose running costs are register pairs (two templates, or two windows): v = d + min3 over
// PT[q] = D[r-1][(r-1-W)+q], one v_pk_add_f32 adds the two v_min3_f32 results.  GUARD: only the first 2W rows can touch columns c < 1 and
// need the +inf guard; columns c > n are never read back by an in-range cell (they only feed cells further right / below-right) and stay
// unguarded.  D: the 2W band costs of the row.  Takes r and W, B from the scope.
#define RP_DTW_MIN_CHAIN2(GUARD, D, PT)                                                                \
    v2f left = (v2f){RP_INF, RP_INF};                                                                  \
    _Pragma("unroll") for (int q = 0; q < B; ++q) {                                                    \
        v2f m;                                                                                         \
        m.x = fminf(fminf((PT)[q + 1].x, left.x), (PT)[q].x);                                          \
        m.y = fminf(fminf((PT)[q + 1].y, left.y), (PT)[q].y);                                          \
        v2f v = (D)[q] + m;                                                                            \
        if (GUARD) v = (r - W + q >= 1) ? v : (v2f){RP_INF, RP_INF};                                   \
        (PT)[q] = v;                                                                                   \
        left = v;                                                                                      \
    }

// ---- the wide row sweep ----------------------------------------------------------------------------------------------------------------------
// Row r of one template, as a body of RP_DTW_ROW_BLOCK: the costs of the 2W band cells are formed two cells per packed FMA
// (d = fma(-a[k], y[k], d) chained from 1, the coefficient duplicated into a scalar pair), then the serial min chain v = d + min3 runs over
// PT[q] = D[r-1][(r-1-W)+q].  GUARD: only the first 2W rows can touch columns c < 1 and need the +inf guard; columns c > n are never read
// back by an in-range cell (they only feed cells further right / below-right) and stay unguarded (the stage holds W frames of slack).
// AROW: the address of coefficient 0 of the template's row r - 1, ES floats from one coefficient to the next.  Takes ring and K, W, B from
// the scope.
#define RP_DTW_WIDE_SWEEP(GUARD, AROW, ES, PT)                                                         \
    {                                                                                                  \
        const float *arow = (AROW);                                                                    \
        v2f dd[B / 2];                                                                                 \
        _Pragma("unroll") for (int j = 0; j < B / 2; ++j) dd[j] = (v2f){1.f, 1.f};                     \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                \
            const v2f a2 = (v2f){arow[(ES) * k], arow[(ES) * k]};                                      \
            _Pragma("unroll") for (int j = 0; j < B / 2; ++j)                                          \
                dd[j] = __builtin_elementwise_fma(-a2, ring[j][k], dd[j]);                             \
        }                                                                                              \
        float left = RP_INF;                                                                           \
        _Pragma("unroll") for (int q = 0; q < B; ++q) {                                                \
            const int slot = (1 + u + q + B - W) % B;                                                  \
            const float d = (slot & 1) ? dd[slot / 2].y : dd[slot / 2].x;                              \
            float v = d + fminf(fminf((PT)[q + 1], left), (PT)[q]);                                    \
            if (GUARD) v = (r - W + q >= 1) ? v : RP_INF;                                              \
            (PT)[q] = v;                                                                               \
            left = v;                                                                                  \
        }                                                                                              \
    }

// ---- abandon guard and epilogue --------------------------------------------------------------------------------------------------------------
// The averaged template (output column T) is never abandoned: its score is reported and gates.  Templates::create gives it a chunk of its
// own, so a kernel may ask it of the chunk (template 0) or of each template.
__device__ __forceinline__ bool dtw_is_averaged(const DtwChunk *ch, int t, int T) { return ch->tid[t] >= T; }

// D[m-1][n] of an m == n == L walk -> cost / (m + n) -> dtw_logistic -> column `tid` of the row's scores, or avg for the averaged template.
// Takes denom = (float)(L + L), score_ref, T, scores, avg from the scope.
#define RP_DTW_STORE_SCORE(cost, TID, row)                                                             \
    do {                                                                                               \
        const float nc = (cost) / denom;                                                               \
        const float sc = dtw_logistic(nc, score_ref);                                                  \
        const int tid_ = (TID);                                                                        \
        if (tid_ < T) scores[(row) * T + tid_] = sc;                                                   \
        else avg[row] = sc;                                                                            \
    } while (0)
// the norm-range test of a finished (or abandoned) window: list (row, chunk) for dtw_ref_kernel.  Takes gl, chunk_base, ci from the scope.
#define RP_DTW_LIST_IF_OUT_OF_RANGE(chk, row)                                                          \
    do {                                                                                               \
        if ((chk) > kDtwFixLimit) dtw_fix_append(gl.fix, row, (uint32_t)(chunk_base + (int)ci));       \
    } while (0)

}  // namespace rp
