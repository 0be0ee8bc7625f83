// rp_dtw.hip -- window scoring: dtw_band_kernel / dtw_band_wide_kernel / dtw_generic_kernel
// (src/mfcc/dtw.rs:56-105 + comparator.rs + normalizer.rs + wakeword_comp.rs:22-27; one lane per window, band and ring
// in registers) and aggregate_kernel (src/wakewords/comp/wakeword_comp.rs:38-49,108-139).  DESIGN.md §4.2.
// The three register kernels share their per-lane walk -- lane -> window maps, column means, ring column load, the wide row sweep, the
// averaged-template guard and the score epilogue -- with each other and with bank_dtw through rp_dtw_lane.h; here each keeps its own tile
// shape, band layout, row body and abandon check.
#include "rp_device.h"
#include "rp_dtw_lane.h"
#include "rp_host.h"

#include <cmath>
#include <cstdlib>

namespace rp {

// -------------------------------------------------------------------------- DTW
// Scoring of one (window, template) pair, reference semantics:
//   window = frames [w, w+L) of the stream (cut to the template length L keeping the
//   OLDEST frames, wakeword_comp.rs:22-27), column-mean normalised (normalizer.rs);
//   D[r][c] = (1 - cos(a[r-1], b[c-1])) + min(D[r-1][c], D[r][c-1], D[r-1][c-1]) on the band
//   c in [r-W, r+W-1]; result D[m-1][n] (dtw.rs:101); score = 1/(1+exp((cost/(m+n)-ref)/ref)).
// Template rows are pre-scaled to unit length on the host and window frames are scaled
// to unit length here, so a cell costs K fused multiply-adds instead of three dot
// products, a sqrt and a divide (comparator.rs:28-48); zero vectors stay zero, which
// reproduces the reference's "magnitude == 0 -> similarity 0".

// One wave = 64 consecutive windows of one stream x one chunk of TC same-length templates.
// Per lane: the window's column means, a ring of the 2W unit-length window frames inside the
// band (shared by all TC templates), and TC bands of 2W+1 running costs held as register pairs of
// two templates: one v_pk_fma_f32 forms the cosine costs of a band cell for both templates (the
// coefficient pair comes from scalar registers, the window component is broadcast by op_sel),
// one v_pk_add_f32 adds the two v_min3_f32 results.  Rows are unrolled 2W at a time so
// every ring slot and band index is a compile-time register.  Only the first 2W rows can touch
// columns c < 1 and need the +inf guard; columns c > n are never read back by an in-range cell
// (they only feed cells further right / below-right), so they are left unguarded.
// GX: lanes read their window's frames straight from global memory instead of an LDS stage: used when a
// stream contributes only a few windows per launch (streaming batches), so that the 64 lanes of a wave
// can belong to many different streams.
template <int K, int W, int TC, bool GX>
__global__ __launch_bounds__(kDtwWin) void dtw_band_kernel(
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_frames_total, unsigned tiles, unsigned n_chunks,
    int chunk_base, size_t first_win, size_t n_win, size_t out_win_pitch, const DtwChunk *__restrict__ chunks,
    const float *__restrict__ dup, int T, float score_ref, float *__restrict__ scores, float *__restrict__ avg,
    int flat, size_t n_streams, GateList gl = GateList{}) {
    constexpr int B = 2 * W;
    constexpr int KP = (K % 2 == 0) ? K + 1 : K;  // odd pitch: conflict-free lane-strided LDS reads
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);  // [64 + 2 (L + W)][KP]: up to two stream segments

    const unsigned tile = blockIdx.x % tiles;
    const unsigned ci = (blockIdx.x / tiles) % n_chunks;
    const int lane = threadIdx.x;
    const DtwChunk *ch = chunks + chunk_base + ci;
    const int L = ch->len;  // m == n == L
    size_t s;
    int w;
    bool valid;
    const float *xl;
    if (GX) {
        static_assert(!GX || KP == K, "global-memory frames have pitch K");
        RP_DTW_GLOBAL_ENTRY(kDtwWin, (size_t)tile * kDtwWin + lane, s, w, valid, xl);
    } else {
        if (gl.count && *gl.count < gl.dense_min) return;  // DENSE mode of the gate: only when (nearly) every window passed
        RP_DTW_STAGE_SEGMENTS(kDtwWin);
        RP_DTW_STAGED_ENTRY(lane, s, w, valid, xl);
    }
    RP_DTW_COL_MEANS();

    RP_DTW_RING_START();  // ring, chk

    // P[tp][q] = D[r-1][(r-1-W)+q] of templates (2tp, 2tp+1); row 0 has D[0][0] = 0 at q = W
    v2f P[TC / 2][B + 1];
#pragma unroll
    for (int t = 0; t < TC / 2; ++t) {
#pragma unroll
        for (int q = 0; q <= B; ++q) P[t][q] = (v2f){RP_INF, RP_INF};
        P[t][W] = (v2f){0.f, 0.f};
    }

    const float *rows = dup + ch->rows_off;
    // row r of every template pair: the pair's coefficients interleaved (t0, t1) per k, one scalar pair; the costs of the 2W band cells first
    // (independent FMA chains, the window component broadcast to both templates), then the serial min chain
#define RP_PAIR_ROWS(GUARD)                                                                            \
    _Pragma("unroll") for (int t = 0; t < TC / 2; ++t) {                                               \
        const v2f *arow = reinterpret_cast<const v2f *>(rows + ((size_t)(r - 1) * (TC / 2) + t) * K * 2); \
        v2f a2[K];                                                                                     \
        _Pragma("unroll") for (int k = 0; k < K; ++k) a2[k] = arow[k];                                 \
        v2f d[B];                                                                                      \
        _Pragma("unroll") for (int q = 0; q < B; ++q) d[q] = (v2f){1.f, 1.f};                          \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                \
            _Pragma("unroll") for (int q = 0; q < B; ++q) {                                            \
                const int slot = (1 + u + q + B - W) % B;                                              \
                const v2f yy = (slot & 1) ? ring[slot / 2][k].yy : ring[slot / 2][k].xx;               \
                d[q] = __builtin_elementwise_fma(-a2[k], yy, d[q]);                                    \
            }                                                                                          \
        }                                                                                              \
        RP_DTW_MIN_CHAIN2(GUARD, d, P[t]);                                                             \
    }
#define RP_ROWS(GUARD) RP_DTW_ROW_BLOCK(RP_DTW_LOAD_COL, RP_PAIR_ROWS(GUARD))

    {
        const int r0 = 1;
        RP_ROWS(true)
    }
    const float abandon_cost = gl.abandon_nc * (float)(L + L);
    for (int r0 = 1 + B; r0 < L; r0 += B) {
        if (gl.abandon_nc < RP_INF) {  // wave-uniform; once per 2W rows
            bool alive = false;
#pragma unroll
            for (int t = 0; t < TC / 2; ++t) {
                v2f m = P[t][0];
#pragma unroll
                for (int q = 1; q < B; ++q) m = (v2f){fminf(m.x, P[t][q].x), fminf(m.y, P[t][q].y)};
                // asked of each template: Templates::create keeps the averaged one out of this kernel's chunks today, the guard keeps
                // that an optimisation
                alive = alive || (2 * t < ch->count && (m.x <= abandon_cost || dtw_is_averaged(ch, 2 * t, T))) ||
                        (2 * t + 1 < ch->count && (m.y <= abandon_cost || dtw_is_averaged(ch, 2 * t + 1, T)));
            }
            if (!__any(alive && valid)) {
                if (valid) {
                    const size_t row = s * out_win_pitch + (size_t)w;
                    for (int t = 0; t < ch->count; ++t)
                        if (!dtw_is_averaged(ch, t, T)) scores[row * T + ch->tid[t]] = 0.f;
                    RP_DTW_LIST_IF_OUT_OF_RANGE(chk, row);
                }
                return;
            }
        }
        RP_ROWS(false)
    }
#undef RP_ROWS
#undef RP_PAIR_ROWS

    if (valid) {
        const size_t row = s * out_win_pitch + (size_t)w;
        const float denom = (float)(L + L);
#pragma unroll
        for (int t = 0; t < TC; ++t) {
            if (t < ch->count) RP_DTW_STORE_SCORE((t & 1) ? P[t / 2][W + 1].y : P[t / 2][W + 1].x, ch->tid[t], row);  // D[m-1][n] for m == n
        }
        RP_DTW_LIST_IF_OUT_OF_RANGE(chk, row);
    }
}

// One template, TWO windows per lane.  A chunk that holds a single template (every template of a ragged reference such as
// the reference's own oye_casa_g.rpw, 108/96/90/93/102 frames; the averaged template) would leave one half of every packed
// instruction of dtw_band_kernel<.., 2> idle.  Here the two halves are two windows: a wave owns 128 consecutive entries
// of the flattened (stream, window) space, lane l entries l and l + 64; means, ring and band are all register pairs,
// the template coefficient is a scalar broadcast to both halves.  Same operations per cell as dtw_band_kernel, same
// bits.  GX / list as there (entries read their frames from global memory).
template <int K, int W, bool GX>
__global__ __launch_bounds__(kDtwWin) void dtw_band2_kernel(
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_frames_total, unsigned tiles, unsigned n_chunks,
    int chunk_base, size_t first_win, size_t n_win, size_t out_win_pitch, const DtwChunk *__restrict__ chunks,
    const float *__restrict__ dup, int T, float score_ref, float *__restrict__ scores, float *__restrict__ avg,
    int flat, size_t n_streams, GateList gl = GateList{}) {
    constexpr int B = 2 * W, NW = 2 * kDtwWin;
    constexpr int KP = (K % 2 == 0) ? K + 1 : K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);  // [128 + 2 (L + W)][KP]: up to two stream segments

    const unsigned tile = blockIdx.x % tiles;
    const unsigned ci = (blockIdx.x / tiles) % n_chunks;
    const int lane = threadIdx.x;
    const DtwChunk *ch = chunks + chunk_base + ci;
    const int L = ch->len;  // m == n == L
    size_t s[2];
    int w[2];
    bool valid[2];
    const float *xl[2];
    if (GX) {
        static_assert(!GX || KP == K, "global-memory frames have pitch K");
        // RP_DTW_GLOBAL_ENTRY for two entries, with the leave tests taken once in front: spelled out, because the macro expanded twice
        // compiles to another prologue (and another register allocation) in the four builds of this branch
        unsigned n_listed = 0;
        if (gl.list) {
            n_listed = *gl.count;
            if ((size_t)tile * NW >= n_listed || (gl.dense_min && n_listed >= gl.dense_min)) return;
        } else if (gl.count && *gl.count < gl.dense_min) return;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            size_t f = (size_t)tile * NW + (size_t)e * kDtwWin + lane;
            if (gl.list) {
                valid[e] = f < n_listed;
                f = gl.list[valid[e] ? f : n_listed - 1];
            } else {
                valid[e] = f < n_streams * n_win;
            }
            s[e] = valid[e] ? f / n_win : 0;
            w[e] = valid[e] ? (int)(f - s[e] * n_win) : 0;
            xl[e] = mfcc + (s[e] * frame_pitch + first_win + (size_t)w[e]) * K;
        }
    } else {
        if (gl.count && *gl.count < gl.dense_min) return;
        RP_DTW_STAGE_SEGMENTS(NW);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int ent = e * kDtwWin + lane;
            RP_DTW_STAGED_ENTRY(ent, s[e], w[e], valid[e], xl[e]);
        }
    }
    const float *x0 = xl[0], *x1 = xl[1];
    RP_DTW_COL_MEANS2();

    v2f ring[B][K];  // ring[slot][k] = unit-length frame of the slot, (window 0, window 1)
#pragma unroll
    for (int j = 0; j < B; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) ring[j][k] = (v2f){0.f, 0.f};

    v2f chk = (v2f){0.f, 0.f};  // the norm-range test of the two windows (RP_DTW_LOAD_COL2)
#pragma unroll
    for (int c = 1; c < W; ++c) RP_DTW_LOAD_COL2(c, c % B);

    v2f P[B + 1];
#pragma unroll
    for (int q = 0; q <= B; ++q) P[q] = (v2f){RP_INF, RP_INF};
    P[W] = (v2f){0.f, 0.f};

    const float *rows = dup + ch->rows_off;  // [len][1][K][2]: the template's coefficients (stored twice)
    // row r: the template's coefficient broadcast to both windows
#define RP_WINDOW_PAIR_ROW(GUARD)                                                                      \
    const float *arow = rows + (size_t)(r - 1) * K * 2;                                                \
    v2f d[B];                                                                                          \
    _Pragma("unroll") for (int q = 0; q < B; ++q) d[q] = (v2f){1.f, 1.f};                              \
    _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                    \
        const float a = arow[2 * k];                                                                   \
        const v2f na = (v2f){-a, -a};                                                                  \
        _Pragma("unroll") for (int q = 0; q < B; ++q)                                                  \
            d[q] = __builtin_elementwise_fma(na, ring[(1 + u + q + B - W) % B][k], d[q]);              \
    }                                                                                                  \
    RP_DTW_MIN_CHAIN2(GUARD, d, P);
#define RP_ROWS2(GUARD) RP_DTW_ROW_BLOCK(RP_DTW_LOAD_COL2, RP_WINDOW_PAIR_ROW(GUARD))
    {
        const int r0 = 1;
        RP_ROWS2(true)
    }
    const int tid = ch->tid[0];
    const float abandon_cost = gl.abandon_nc * (float)(L + L);
    for (int r0 = 1 + B; r0 < L; r0 += B) {
        if (gl.abandon_nc < RP_INF && !dtw_is_averaged(ch, 0, T)) {  // asked of the chunk: it is one template
            v2f m = P[0];
#pragma unroll
            for (int q = 1; q < B; ++q) m = (v2f){fminf(m.x, P[q].x), fminf(m.y, P[q].y)};
            const bool alive = (valid[0] && m.x <= abandon_cost) || (valid[1] && m.y <= abandon_cost);
            if (!__any(alive)) {
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    if (valid[e]) {
                        scores[(s[e] * out_win_pitch + (size_t)w[e]) * T + tid] = 0.f;
                        RP_DTW_LIST_IF_OUT_OF_RANGE(e ? chk.y : chk.x, s[e] * out_win_pitch + (size_t)w[e]);
                    }
                return;
            }
        }
        RP_ROWS2(false)
    }
#undef RP_ROWS2
#undef RP_WINDOW_PAIR_ROW

    const float denom = (float)(L + L);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (valid[e]) {
            const size_t row = s[e] * out_win_pitch + (size_t)w[e];
            RP_DTW_STORE_SCORE(e ? P[W + 1].y : P[W + 1].x, tid, row);  // D[m-1][n] for m == n
            RP_DTW_LIST_IF_OUT_OF_RANGE(e ? chk.y : chk.x, row);
        }
    }
}

// Variant for wide frames (K = 16): the ring alone is 160 registers, so the band costs are formed one
// template at a time with two band cells per v_pk_fma_f32 (coefficient duplicated into a scalar pair)
// instead of holding the costs of a template pair for all 2W cells.
template <int K, int W, int TC, bool GX = false>
__global__ __launch_bounds__(kDtwWin) void dtw_band_wide_kernel(
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_frames_total, unsigned tiles, unsigned n_chunks,
    int chunk_base, size_t first_win, size_t n_win, size_t out_win_pitch, const DtwChunk *__restrict__ chunks,
    const float *__restrict__ dup, int T, float score_ref, float *__restrict__ scores, float *__restrict__ avg,
    size_t n_streams = 0, GateList gl = GateList{}) {
    constexpr int B = 2 * W;
    constexpr int TP = TC >= 2 ? TC / 2 : 1;      // template pairs per row of `dup` (a one-template chunk is stored as a pair)
    // LDS rows get an odd pitch (conflict-free lane-strided reads); GX lanes read rows of pitch K from global memory
    constexpr int KP = GX ? K : ((K % 2 == 0) ? K + 1 : K);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);  // [64 + L + W][KP]

    const unsigned tile = blockIdx.x % tiles;
    const unsigned ci = (blockIdx.x / tiles) % n_chunks;
    const int lane = threadIdx.x;
    const DtwChunk *ch = chunks + chunk_base + ci;
    const int L = ch->len;  // m == n == L
    size_t s;
    size_t wl;      // window index of this lane inside its stream
    bool valid;
    const float *xl;
    if (GX) {
        RP_DTW_GLOBAL_ENTRY(kDtwWin, (size_t)tile * kDtwWin + lane, s, wl, valid, xl);
    } else {
        // one stream segment of a whole tile's 64 + L + W frames, never flat: not RP_DTW_STAGE_SEGMENTS (it stages n + L + W frames of up
        // to two segments, which is another instruction stream)
        if (gl.count && *gl.count < gl.dense_min) return;
        s = blockIdx.x / ((size_t)tiles * n_chunks);
        const size_t w0 = first_win + (size_t)tile * kDtwWin;
        const int n_stage = kDtwWin + L + W;
        const float *src = mfcc + s * frame_pitch * K;
        for (int i = lane; i < n_stage * K; i += kDtwWin) {
            int f = i / K, k = i - f * K;
            size_t g = w0 + f;
            xs[f * KP + k] = g < n_frames_total ? src[g * K + k] : 0.f;
        }
        __syncthreads();
        wl = (size_t)tile * kDtwWin + lane;
        valid = wl < n_win;
        xl = xs + lane * KP;
    }
    RP_DTW_COL_MEANS();

    RP_DTW_RING_START();  // ring, chk

    // P[t][q] = D[r-1][(r-1-W)+q] of template t; row 0 has D[0][0] = 0 at q = W
    float P[TC][B + 1];
#pragma unroll
    for (int t = 0; t < TC; ++t) {
#pragma unroll
        for (int q = 0; q <= B; ++q) P[t][q] = RP_INF;
        P[t][W] = 0.f;
    }

    // template t's row: coefficient k of the pair (t / 2) at [2 k + (t & 1)] of the interleaved pair row
    const float *rows = dup + ch->rows_off;
#define RP_ROWS(GUARD)                                            \
    RP_DTW_ROW_BLOCK(RP_DTW_LOAD_COL, _Pragma("unroll") for (int t = 0; t < TC; ++t) \
                     RP_DTW_WIDE_SWEEP(GUARD, rows + ((size_t)(r - 1) * TP + t / 2) * K * 2 + (t & 1), 2, P[t]))
    {
        const int r0 = 1;
        RP_ROWS(true)
    }
    const float abandon_cost = gl.abandon_nc * (float)(L + L);
    for (int r0 = 1 + B; r0 < L; r0 += B) {
        if (gl.abandon_nc < RP_INF && !dtw_is_averaged(ch, 0, T)) {  // asked of the chunk: the averaged template has one of its own
            bool alive = false;
#pragma unroll
            for (int t = 0; t < TC; ++t) {
                float m = P[t][0];
#pragma unroll
                for (int q = 1; q < B; ++q) m = fminf(m, P[t][q]);
                alive = alive || (t < ch->count && m <= abandon_cost);
            }
            if (!__any(alive && valid)) {
                if (valid) {
                    for (int t = 0; t < ch->count; ++t) scores[(s * out_win_pitch + wl) * T + ch->tid[t]] = 0.f;
                    RP_DTW_LIST_IF_OUT_OF_RANGE(chk, s * out_win_pitch + wl);
                }
                return;
            }
        }
        RP_ROWS(false)
    }
#undef RP_ROWS

    if (valid) {
        const size_t row = s * out_win_pitch + wl;
        const float denom = (float)(L + L);
#pragma unroll
        for (int t = 0; t < TC; ++t) {
            if (t < ch->count) RP_DTW_STORE_SCORE(P[t][W + 1], ch->tid[t], row);  // D[m-1][n] for m == n
        }
        RP_DTW_LIST_IF_OUT_OF_RANGE(chk, row);
    }
}

// Fallback for any K / band size / m != n: one wave = 64 windows x one template, band
// and column means in LDS (lane-minor, conflict-free), costs evaluated per cell.
__global__ __launch_bounds__(64) void dtw_generic_kernel(
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_frames_total, unsigned tiles, size_t first_win,
    size_t n_win, size_t out_win_pitch, const int *__restrict__ lens, const float *__restrict__ unit, int Lpad, int K,
    int T, int t_first, int t_count, int max_len, int band, float score_ref, float *__restrict__ scores, float *__restrict__ avg,
    const float *gate_avg, float gate_threshold, uint32_t *__restrict__ fix) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int KP = K | 1;
    const unsigned tile = blockIdx.x % tiles;
    const int t = t_first + (int)((blockIdx.x / tiles) % t_count);   // templates t_first .. t_first + t_count - 1 (T = the averaged one)
    const size_t s = blockIdx.x / ((size_t)tiles * t_count);
    const int lane = threadIdx.x;
    // the averaged-template gate (wakeword_comp.rs:85-93) at wave granularity: when none of the wave's 64 windows passed it,
    // the sample templates are not compared at all; a wave with a passing window scores all of its windows and the
    // aggregate pass writes 0 for the rejected ones, so both cases leave the same aggregates
    if (gate_avg) {
        const size_t wl = (size_t)tile * 64 + lane;
        const bool pass = wl < n_win && !(gate_avg[s * out_win_pitch + wl] < gate_threshold);
        if (!__any(pass)) return;
    }
    const size_t w0 = first_win + (size_t)tile * 64;
    const int m = lens[t];
    const int n = m < max_len ? m : max_len;  // window cut to the template length
    const int diff = m > n ? m - n : n - m;
    const int W = band > diff ? band : diff;
    const int B = 2 * W;

    const int n_stage = 64 + max_len - 1;
    float *xs = reinterpret_cast<float *>(smem);      // [n_stage][KP]
    float *mus = xs + (size_t)n_stage * KP;           // [K][64]
    float *Pb = mus + (size_t)K * 64;                 // [B+1][64]
    const float *src = mfcc + s * frame_pitch * K;
    for (int i = lane; i < n_stage * K; i += 64) {
        int f = i / K, k = i - f * K;
        size_t g = w0 + f;
        xs[f * KP + k] = g < n_frames_total ? src[g * K + k] : 0.f;
    }
    __syncthreads();
    const float *xl = xs + lane * KP;
    for (int k = 0; k < K; ++k) {
        float sum = 0.f;
        for (int i = 0; i < n; ++i) sum += xl[i * KP + k];
        mus[k * 64 + lane] = sum / (float)n;
    }
    for (int q = 0; q <= B; ++q) Pb[q * 64 + lane] = RP_INF;
    Pb[W * 64 + lane] = 0.f;
    const float *trow = unit + (size_t)t * Lpad * K;
    float chk = 0.f;  // the norm-range test (see dtw_band_kernel)
    for (int r = 1; r < m; ++r) {
        float left = RP_INF;
        for (int q = 0; q < B; ++q) {
            const int c = r - W + q;
            float v = RP_INF;
            if (c >= 1 && c <= n) {
                // the arithmetic of the register kernels, operation for operation (unit-length frame first, then
                // d = 1 - a.y as one fma chain from 1): every DTW kernel gives the same bits for the same window
                float bb = 0.f;
                for (int k = 0; k < K; ++k) {
                    const float y = xl[(c - 1) * KP + k] - mus[k * 64 + lane];
                    bb = fmaf(y, y, bb);
                }
                const float inv = bb > 0.f ? rsqrtf(bb) : 0.f;
                chk = fmaxf(fmaxf(chk, inv), bb);
                float d = 1.f;
                for (int k = 0; k < K; ++k) {
                    const float y = (xl[(c - 1) * KP + k] - mus[k * 64 + lane]) * inv;
                    d = fmaf(-trow[(r - 1) * K + k], y, d);
                }
                v = d + fminf(fminf(Pb[(q + 1) * 64 + lane], left), Pb[q * 64 + lane]);
            }
            Pb[q * 64 + lane] = v;
            left = v;
        }
    }
    if (tile * (size_t)64 + lane < n_win) {
        const int qs = n - (m - 1 - W);  // column n of row m-1
        float cost = (qs >= 0 && qs < B) ? Pb[qs * 64 + lane] : RP_INF;
        float nc = cost / (float)(m + n);
        float sc = dtw_logistic(nc, score_ref);
        size_t row = s * out_win_pitch + (size_t)tile * 64 + lane;
        if (t < T) scores[row * T + t] = sc;
        else avg[row] = sc;
        if (chk > kDtwFixLimit) dtw_fix_append(fix, row, kFixSpecTemplate | (uint32_t)t);
    }
}

// ---- the reference-shaped cell (comparator.rs:28-48) for what the scale-invariant kernels cannot reproduce ------------------
// dot_ab / sqrt(dot_a * dot_b) in f32 with `== 0 -> 0`: when the PRODUCT of the two squared norms underflows the reference's
// similarity becomes 0 (distance 1) although neither vector is zero, when it is subnormal the quotient loses bits, when it
// overflows the similarity is 0 again.  Every fast kernel lists the (window, chunk or template) pairs that met a frame outside
// kDtwNormLo..kDtwFixLimit (DtwWork::fix); this kernel rescores them cell by cell as the reference does -- three sequential dot
// products of the template row AS GIVEN and the mean-normalised frame, one sqrt, one divide -- and overwrites their scores.
// One lane per listed pair (a chunk's templates one after the other); frames and rows come from global memory, band and means
// sit in LDS lane-minor.  ALL mode (force_all, or more pairs than the list holds): every window x templates t_first ..
// t_first + t_count - 1 (template sets with a row outside kDtwNormLo..kDtwNormHiRow, TemplatesDev::ref_only).  agg_out: the pair's
// chunk holds every sample template (DtwFusedAgg) -- ScoreMode::Max and the stream's hot flag are rewritten too.
// Launched after the fast kernels of every call; without listed pairs each workgroup reads one word and leaves.  Otherwise the
// last workgroup to leave puts fix[0] and fix[1] back to zero.
__global__ __launch_bounds__(64) void dtw_ref_kernel(
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_frames_total, size_t first_win, size_t n_win, size_t out_win_pitch,
    size_t n_streams, const int *__restrict__ lens, const float *__restrict__ raw, int Lpad, int K, int T, int max_len, int band, int Wmax,
    float score_ref, const DtwChunk *__restrict__ chunks, float *__restrict__ scores, float *__restrict__ avg, uint32_t *fix,
    int force_all, int t_first, int t_count, float *__restrict__ agg_out, uint32_t *__restrict__ agg_hot, float agg_threshold) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *mus = reinterpret_cast<float *>(smem);  // [K][64]
    float *Pb = mus + (size_t)K * 64;              // [2 Wmax + 1][64]
    const int lane = threadIdx.x;
    const uint32_t n_listed = fix[0];
    // nothing listed (every call on ordinary audio): leave without touching the counters -- 512 workgroups adding to one word
    // took 11 us, as long as a twentieth of a live-stream call's DTW launch.  With a list every workgroup sees the same non-zero
    // count (nobody resets it before all have checked in), so either all run the protocol below or none does.
    if (!force_all && n_listed == 0) return;
    const bool all = force_all || n_listed > kDtwFixCap;
    const size_t per_row = agg_out ? 1 : (size_t)t_count;
    const size_t n_entries = all ? n_streams * n_win * per_row : (size_t)n_listed;
    const unsigned long long *list = reinterpret_cast<const unsigned long long *>(fix + 2);
    if (blockIdx.x == 0 && lane == 0 && n_entries) atomicAdd(dtw_fix_stats(fix), (unsigned long long)n_entries);  // rp_ctx_dtw_ref_pairs
    for (size_t e = (size_t)blockIdx.x * 64 + lane; e < n_entries; e += (size_t)gridDim.x * 64) {
        size_t row;
        int tb, te, from_chunk = -1;   // templates tb .. te - 1, or the tid[] of chunk from_chunk
        if (all) {
            const size_t rw = e / per_row;
            const size_t s_ = rw / n_win;
            row = s_ * out_win_pitch + (rw - s_ * n_win);
            if (agg_out) { tb = t_first; te = t_first + t_count; }
            else { tb = t_first + (int)(e - rw * per_row); te = tb + 1; }
        } else {
            const unsigned long long v = list[e];
            row = (size_t)(v >> 24);
            const uint32_t spec = (uint32_t)v & kFixSpecMask;
            if (spec & kFixSpecTemplate) { tb = (int)(spec & (kFixSpecTemplate - 1)); te = tb + 1; }
            else { from_chunk = (int)spec; tb = 0; te = chunks[from_chunk].count; }
        }
        const size_t s = row / out_win_pitch, w = row - s * out_win_pitch;
        const size_t f0 = s * frame_pitch + first_win + w;       // the window's first frame
        const float *xw = mfcc + f0 * K;   // only columns 1..n are read: the window's own frames
        float best = 0.f;
        int mean_n = -1;
        for (int ti = tb; ti < te; ++ti) {
            const int t = from_chunk >= 0 ? chunks[from_chunk].tid[ti] : ti;
            const int m = lens[t];
            const int n = m < max_len ? m : max_len;  // window cut to the template length (wakeword_comp.rs:22-27)
            const int diff = m > n ? m - n : n - m;
            const int W = band > diff ? band : diff;  // dtw.rs:64-67
            const int B = 2 * W;
            if (n != mean_n) {  // MfccNormalizer::normalize (normalizer.rs:17-29): sequential column sums over the n frames
                for (int k = 0; k < K; ++k) {
                    float sum = 0.f;
                    for (int i = 0; i < n; ++i) sum += xw[(size_t)i * K + k];
                    mus[k * 64 + lane] = sum / (float)n;
                }
                mean_n = n;
            }
            for (int q = 0; q <= B; ++q) Pb[q * 64 + lane] = RP_INF;
            Pb[W * 64 + lane] = 0.f;
            const float *trow = raw + (size_t)t * Lpad * K;
            for (int r = 1; r < m; ++r) {   // rows 1..m-1: row m is never read (dtw.rs:101)
                float left = RP_INF;
                for (int q = 0; q < B; ++q) {
                    const int c = r - W + q;
                    float v = RP_INF;
                    if (c >= 1 && c <= n) {
                        float dot_ab = 0.f, dot_a = 0.f, dot_b = 0.f;
                        for (int k = 0; k < K; ++k) {
                            const float ca = trow[(r - 1) * K + k];
                            const float cb = xw[(size_t)(c - 1) * K + k] - mus[k * 64 + lane];
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
            const int qs = n - (m - 1 - W);  // column n of row m-1
            const float cost = (qs >= 0 && qs < B) ? Pb[qs * 64 + lane] : RP_INF;
            const float nc = cost / (float)(m + n);
            const float sc = dtw_logistic(nc, score_ref);
            if (t < T) { scores[row * T + t] = sc; best = fmaxf(best, sc); }
            else avg[row] = sc;
        }
        if (agg_out) {
            agg_out[row] = best;
            if (agg_hot && best > agg_threshold) agg_hot[s] = 1u;
        }
    }
    __syncthreads();
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(fix + 1, 1u) == gridDim.x - 1) { fix[0] = 0; fix[1] = 0; }
    }
}

// A launcher that fails between its fast kernels and the list pass must not leave pairs of THIS call (rows of these arrays) listed for
// the next one: the call's words go back to zero behind whatever was already queued.  Returns the error it was given.
static hipError_t dtw_abort(hipStream_t st, const DtwWork &wk, hipError_t e) {
    if (wk.fix) (void)hipMemsetAsync(wk.fix, 0, 2 * sizeof(uint32_t), st);
    if (wk.sched) (void)hipMemsetAsync(wk.sched, 0, 2 * (size_t)kDtwSchedChunks * sizeof(uint32_t), st);
    (void)hipGetLastError();
    return e;
}

// The pass behind every fast launch: rescoring of the listed pairs (see dtw_ref_kernel).  force_all: every window x templates
// t_first .. t_first + t_count - 1 (index T = the averaged template).
static hipError_t launch_dtw_ref(const DtwCall &c, bool force_all, int t_first, int t_count, const DtwFusedAgg *fuse = nullptr) {
    const TemplatesDev &t = *c.t;
    if (!c.wk.fix || !t.raw) return hipErrorInvalidValue;
    const int Wmax = c.band > t.max_diff ? c.band : t.max_diff;
    const size_t lds = ((size_t)t.K * 64 + (size_t)(2 * Wmax + 1) * 64) * sizeof(float);
    if (lds > 160 * 1024) return hipErrorMemoryAllocation;
    if (lds > 64 * 1024)
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(dtw_ref_kernel), 160 * 1024); e != hipSuccess) return e;
    // list mode: four workgroups per CU -- with nothing listed each reads one word and leaves; with more pairs than the list holds
    // (kDtwFixCap: pathological input) the kernel falls back to every window of the call, and a grid of one workgroup per CU would
    // walk them sixteen thousand lanes wide
    size_t blocks = 4 * (size_t)device_cu_count();
    if (force_all) dtw_mark(c.wk, kDtwRanRefAll);
    if (force_all) {
        const size_t need = (c.S * c.n_win * (size_t)(fuse ? 1 : t_count) + 63) / 64;
        blocks = need < 8 * (size_t)device_cu_count() ? (need ? need : 1) : 8 * (size_t)device_cu_count();
    }
    const bool fused = fuse && fuse->agg;
    hipLaunchKernelGGL(dtw_ref_kernel, dim3((unsigned)blocks), dim3(64), lds, c.st, c.mfcc, c.frame_pitch, c.frame_pitch, c.first_win, c.n_win,
                       c.out_win_pitch, c.S, t.lens, t.raw, t.Lpad, t.K, t.T, t.max_len, c.band, Wmax, c.score_ref, t.chunks, c.scores, c.avg, c.wk.fix,
                       force_all ? 1 : 0, t_first, t_count, fused ? fuse->agg : nullptr, fused ? fuse->hot : nullptr, fused ? fuse->threshold : 0.f);
    return hipGetLastError();
}

// Grid of one register-kernel launch over n_chunks chunks, NW windows per wave.  from_global (streams contribute fewer windows than a wave
// holds, or the windows come from the gate's list): the lanes of a wave are consecutive entries of the flattened (stream, window) space --
// of the list, list_mult entries per row -- and read their frames from global memory (the caller guarantees W*K floats of slack after the
// last stream's frames).  Staged: the same flattened tiling when the kernel knows it (may_flat) and every stream has at least one full
// tile of windows, else tiles that never cross a stream.
struct BandGrid {
    int flat = 0;
    unsigned ft = 0, blocks = 0;   // tiles (flat: of the call, else of one stream), workgroups
};
static hipError_t dtw_band_grid(const DtwCall &c, size_t NW, int n_chunks, bool from_global, size_t list_mult, bool may_flat, BandGrid &g) {
    g.flat = (from_global || (may_flat && c.n_win >= NW && c.S > 1)) ? 1 : 0;
    const size_t ft = g.flat ? (c.S * c.n_win * list_mult + NW - 1) / NW : (c.n_win + NW - 1) / NW;
    const size_t blocks = ft * (size_t)n_chunks * (g.flat ? 1 : c.S);
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    g.ft = (unsigned)ft;
    g.blocks = (unsigned)blocks;
    return hipSuccess;
}
// LDS of a staged register launch: a wave's NW windows and `segs` stream segments of max_len + W frames, pitch mfcc_size | 1
static hipError_t dtw_band_lds(const DtwCall &c, const void *kernel, int NW, int segs, int W, size_t &lds) {
    lds = (size_t)(NW + segs * (c.t->max_len + W)) * (size_t)(c.t->K | 1) * sizeof(float);
    return lds > 64 * 1024 ? allow_dynamic_lds(kernel, 160 * 1024) : hipSuccess;
}

// dtw_band_kernel (NW = 64 windows per wave) or dtw_band2_kernel (128: chunks of ONE template, two windows per lane) at mfcc_size 5 over
// chunks chunk_base .. chunk_base + n_chunks - 1: `global` is the kernel's form that reads frames from global memory (mfcc_size 5 is odd:
// the pitch of the frames in memory is the conflict-free one), `staged` the LDS-staged form
using BandKernel = void (*)(const float *, size_t, size_t, unsigned, unsigned, int, size_t, size_t, size_t, const DtwChunk *, const float *, int,
                            float, float *, float *, int, size_t, GateList);
static hipError_t launch_dtw_band(const DtwCall &c, int NW, int W, BandKernel global, BandKernel staged, int chunk_base, int n_chunks, bool few,
                                  GateList gl) {
    if (n_chunks <= 0) return hipSuccess;
    dtw_mark(c.wk, kDtwRanRegister);
    const TemplatesDev &t = *c.t;
    gl.fix = c.wk.fix;
    const bool from_global = few || gl.list;
    const BandKernel kernel = from_global ? global : staged;
    BandGrid g;
    if (hipError_t e = dtw_band_grid(c, (size_t)NW, n_chunks, from_global, gl.list ? (size_t)gl.list_mult : 1, true, g); e != hipSuccess) return e;
    size_t lds = 0;
    if (!from_global)
        if (hipError_t e = dtw_band_lds(c, reinterpret_cast<const void *>(staged), NW, 2, W, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(kDtwWin), lds, c.st, c.mfcc, c.frame_pitch, c.frame_pitch, g.ft,
                       (unsigned)n_chunks, chunk_base, c.first_win, c.n_win, c.out_win_pitch, t.chunks, t.dup, t.T, c.score_ref, c.scores, c.avg,
                       g.flat, c.S, gl);
    return hipGetLastError();
}
template <int W, int TC>
static hipError_t launch_dtw_class(const DtwCall &c, int chunk_base, int n_chunks, bool few, const GateList &gl) {
    return launch_dtw_band(c, kDtwWin, W, dtw_band_kernel<5, W, TC, true>, dtw_band_kernel<5, W, TC, false>, chunk_base, n_chunks, few, gl);
}
template <int W>
static hipError_t launch_dtw_single_chunks(const DtwCall &c, int chunk_base, int n_chunks, bool few, const GateList &gl) {
    return launch_dtw_band(c, 2 * kDtwWin, W, dtw_band2_kernel<5, W, true>, dtw_band2_kernel<5, W, false>, chunk_base, n_chunks, few, gl);
}

// dtw_band_wide_kernel (mfcc_size 13 / 16): no flattened staged tiling, one stream segment per staged tile.  (Its list-mode grid covers
// S x n_win entries, not list_mult times as many: it is only reached with list_mult == 1 -- dtw_ragged_kernel, mfcc_size 5, alone
// lists a row more than once.)
template <int K, int W, int TC>
static hipError_t launch_dtw_wide(const DtwCall &c, int chunk_base, int n_chunks, bool few, GateList gl) {
    if (n_chunks <= 0) return hipSuccess;
    dtw_mark(c.wk, kDtwRanRegister);
    const TemplatesDev &t = *c.t;
    gl.fix = c.wk.fix;
    const bool from_global = few || gl.list;
    const auto kernel = from_global ? dtw_band_wide_kernel<K, W, TC, true> : dtw_band_wide_kernel<K, W, TC, false>;
    BandGrid g;
    if (hipError_t e = dtw_band_grid(c, (size_t)kDtwWin, n_chunks, from_global, 1, false, g); e != hipSuccess) return e;
    size_t lds = 0;
    if (!from_global)
        if (hipError_t e = dtw_band_lds(c, reinterpret_cast<const void *>(kernel), kDtwWin, 1, W, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(kDtwWin), lds, c.st, c.mfcc, c.frame_pitch, c.frame_pitch, g.ft, (unsigned)n_chunks, chunk_base,
                       c.first_win, c.n_win, c.out_win_pitch, t.chunks, t.dup, t.T, c.score_ref, c.scores, c.avg, from_global ? c.S : (size_t)0, gl);
    return hipGetLastError();
}

// the averaged template alone: the last of the single-template chunks (class 3)
template <int K, int W>
static hipError_t launch_dtw_avg_chunk(const DtwCall &c, bool few, const GateList &gl) {
    const int avg_chunk = c.t->class_first[3] + c.t->class_count[3] - 1;
    if constexpr (K == 5) return launch_dtw_single_chunks<W>(c, avg_chunk, 1, few, gl);
    else return launch_dtw_wide<K, W, 1>(c, avg_chunk, 1, few, gl);
}

// wide frames (mfcc_size 13 / 16): single-template chunks (class 3, n1 of them) one template per lane, pairs (class 0) two
template <int K, int W>
static hipError_t launch_dtw_wide_all(const DtwCall &c, int n1, bool few, const GateList &gl) {
    const TemplatesDev &t = *c.t;
    // every length at least three times, band 5, rows with slack behind them: the sample templates on the matrix cores
    // (rp_dtw_mfma_wide.hip), the averaged template -- if it is to be scored here -- through the one-template register kernel
    const bool rows_ok = W == 5 && (c.padded_rows || few || gl.list);
    const bool three_part = rows_ok && dtw_mfma_wide3_supported(t, W);                         // the default arithmetic: chunks of four
    const bool two_part = rows_ok && !three_part && dtw_mfma_wide_supported(t, W, c.score_ref);  // RP_ARITH_FAST_SPLIT: chunks of eight
    if (three_part || two_part) {
        if (t.has_avg && n1 == t.class_count[3])
            if (hipError_t e = launch_dtw_avg_chunk<K, W>(c, few, gl); e != hipSuccess) return e;
        return (three_part ? launch_dtw_mfma_wide3 : launch_dtw_mfma_wide)(c, gl);
    }
    if (hipError_t e = launch_dtw_wide<K, W, 1>(c, t.class_first[3], n1, few, gl); e != hipSuccess) return e;
    return launch_dtw_wide<K, W, 2>(c, t.class_first[0], t.class_count[0], few, gl);
}

// ---- one DTW per wave, for a handful of windows (the single-stream API: three new windows per 30 ms chunk) -----
// The register kernels above give every lane a whole DTW: with 3 windows x 5 templates that is 15 busy lanes walking
// ~100 dependent rows each (35 us).  Here a workgroup of one wave owns ONE (window, template) pair: all 64 lanes
// normalise the window and form the band's cosine costs, then the 2W lanes of the band walk the recurrence along
// anti-diagonals (lane q handles band offset q; cell (r, q) is due at step 2r + q, when its left neighbour -- lane q-1,
// one step ago -- and its upper neighbour -- lane q+1, one step ago -- are one DPP lane shift away).  Same operations
// per cell as dtw_band_kernel, same results.
__global__ __launch_bounds__(64) void dtw_single_kernel(
    const float *__restrict__ mfcc, size_t n_frames_total, size_t first_win, unsigned n_win, size_t out_win_pitch,
    const int *__restrict__ lens, const float *__restrict__ unit, int Lpad, int K, int T, int t_first, int t_count, int max_len, int W,
    float score_ref, float *__restrict__ scores, float *__restrict__ avg, const float *__restrict__ raw, int force_ref, uint32_t *fix) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const unsigned wi = blockIdx.x / t_count;
    const int t = t_first + (int)(blockIdx.x - wi * t_count);
    const int m = lens[t];
    const int L = m < max_len ? m : max_len;  // m == n == L (checked by the launcher): the window is cut to L frames
    const int B = 2 * W, KP = K | 1;
    float *ys = reinterpret_cast<float *>(smem);   // [L][KP] window frames, then normalised in place
    float *mu = ys + (size_t)L * KP;               // [K]
    float *dm = mu + ((K + 3) & ~3);               // [2L + B + 16][B] band costs by due step
    float *ts = dm + (size_t)(2 * L + B + 16) * B;                // [L][KP] unit template rows (one coalesced read instead of a
                                                   // dependent global load per multiply-add in the cost loop)
    const float *src = mfcc + (first_win + wi) * (size_t)K;
    const float *trow = unit + (size_t)t * Lpad * K;
    for (int i = lane; i < L * K; i += 64) {
        const int f = i / K, k = i - f * K;
        ys[f * KP + k] = (first_win + wi + f) < n_frames_total ? src[(size_t)f * K + k] : 0.f;
        ts[f * KP + k] = trow[i];
    }
    __syncthreads();
    // MfccNormalizer::normalize: sequential column sums (one lane per coefficient), like the register kernels
    for (int k = lane; k < K; k += 64) {
        float sum = 0.f;
        int i = 0;
        for (; i + 8 <= L; i += 8) {  // eight reads in flight, the adds stay in frame order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ys[(i + j) * KP + k];
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += v[j];
        }
        for (; i < L; ++i) sum += ys[i * KP + k];
        mu[k] = sum / (float)L;
    }
    __syncthreads();
    // the norm-range test of the batch kernels (dtw_band_kernel), healed in place: when a frame of the window leaves
    // kDtwNormLo..kDtwFixLimit (or the template set has such a row: force_ref) this wave forms its costs as the reference does
    // (comparator.rs:28-48) from the rows as given and the centred frames -- the one-wave-per-DTW form has no second pass
    float chk = 0.f;
    for (int f = lane; f < L; f += 64) {
        float bb = 0.f;
        for (int k = 0; k < K; ++k) { const float y = ys[f * KP + k] - mu[k]; bb = fmaf(y, y, bb); }
        chk = fmaxf(fmaxf(chk, bb > 0.f ? rsqrtf(bb) : 0.f), bb);
    }
    const bool ref_cell = force_ref || __any(chk > kDtwFixLimit);
    if (ref_cell && lane == 0) atomicAdd(dtw_fix_stats(fix), 1ull);
    for (int f = lane; f < L; f += 64) {
        float bb = 0.f;
        for (int k = 0; k < K; ++k) { const float y = ys[f * KP + k] - mu[k]; bb = fmaf(y, y, bb); }
        const float inv = ref_cell ? 1.f : (bb > 0.f ? rsqrtf(bb) : 0.f);
        for (int k = 0; k < K; ++k) ys[f * KP + k] = (ys[f * KP + k] - mu[k]) * inv;
    }
    if (ref_cell) {
        const float *rrow = raw + (size_t)t * Lpad * K;
        for (int i = lane; i < L * K; i += 64) { const int f = i / K; ts[f * KP + (i - f * K)] = rrow[i]; }
    }
    __syncthreads();
    // band costs d[r][q] = 1 - a_r . y_c, c = r - W + q, stored by the step they are due at: dm[(2r + q)*B + q];
    // cells outside 1 <= c <= n are never part of a path (+inf)
    const int steps = 2 * (L - 1) + B;  // due steps run from 2 to steps - 1
    for (int i = lane; i < (L - 1) * B; i += 64) {
        const int r = 1 + i / B, q = i - (r - 1) * B, c = r - W + q;
        float d = RP_INF;
        if (c >= 1 && c <= L) {
            const float *a = ts + (r - 1) * KP, *y = ys + (c - 1) * KP;
            if (!ref_cell) {
                d = 1.f;
                for (int k = 0; k < K; ++k) d = fmaf(-a[k], y[k], d);
            } else {
                float dot_ab = 0.f, dot_a = 0.f, dot_b = 0.f;
                for (int k = 0; k < K; ++k) { dot_ab += a[k] * y[k]; dot_a += a[k] * a[k]; dot_b += y[k] * y[k]; }
                const float magnitude = sqrtf(dot_a * dot_b);
                d = 1.f - (magnitude == 0.f ? 0.f : dot_ab / magnitude);
            }
        }
        dm[(2 * r + q) * B + q] = d;
    }
    __syncthreads();
    if (lane >= 16) return;  // the band lives in one DPP row
    const int q = lane < B ? lane : B - 1;
    const bool band_lane = lane < B;
    float cur = lane == W ? 0.f : RP_INF;  // row 0: D[0][0] = 0 sits at band offset W
    const int first_due = q + 2, last_due = 2 * (L - 1) + q;
    const float *dq = dm + q;
    for (int tau0 = 2; tau0 < steps; tau0 += 16) {
        float dreg[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) dreg[j] = dq[(tau0 + j) * B];  // 16 steps' worth of costs, one wait
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int tau = tau0 + j;
            const int ci = __float_as_int(cur);
            const float left = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(RP_INF), ci, 0x111, 0xf, 0xf, false));  // row_shr:1
            // row_shl:1; lane B (never due) stays +inf, so the last band lane's upper neighbour is out of band by itself
            const float up = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(RP_INF), ci, 0x101, 0xf, 0xf, false));
            const bool due = band_lane && ((tau - q) & 1) == 0 && tau >= first_due && tau <= last_due;
            const float nv = dreg[j] + fminf(fminf(up, left), cur);
            cur = due ? nv : cur;
        }
    }
    if (lane == W + 1) {  // D[m-1][n]
        const float nc = cur / (float)(L + L);
        const float sc = dtw_logistic(nc, score_ref);
        const size_t row = (size_t)wi;  // S == 1
        if (t < T) scores[row * T + t] = sc;
        else avg[row] = sc;
    }
}

// Largest template tile the register kernels are built for at this (mfcc_size, band) (0 = only the generic
// kernel applies).  Built: mfcc_size 5 with band 3..6 (tile 8), mfcc_size 13 and 16 with band 3..6 (tile 2).
int dtw_register_tile(int K, int band) {
    if (K == 5 && band >= 3 && band <= 6) return 8;
    if ((K == 13 || K == 16) && band >= 3 && band <= 6) return 2;
    return 0;
}

// dtw_single_kernel over the call's windows (one stream) x templates t_first .. t_first + t_count - 1; lds: DtwRoute::single_lds
static hipError_t launch_dtw_single(const DtwCall &c, size_t lds, int t_first, int t_count) {
    const TemplatesDev &t = *c.t;
    hipLaunchKernelGGL(dtw_single_kernel, dim3((unsigned)(c.n_win * t_count)), dim3(64), lds, c.st, c.mfcc, c.frame_pitch, c.first_win,
                       (unsigned)c.n_win, c.out_win_pitch, t.lens, t.unit, t.Lpad, t.K, t.T, t_first, t_count, t.max_len, c.band, c.score_ref,
                       c.scores, c.avg, t.raw, t.ref_only, c.wk.fix);
    return hipGetLastError();
}

template <int W>
static hipError_t launch_dtw_k5(const DtwCall &c, int n1, bool few, const GateList &gl) {
    const TemplatesDev &t = *c.t;
    const size_t S = c.S, n_win = c.n_win;
    hipError_t e;
    // templates whose length occurs once or twice: the matrix-core kernel for unequal lengths (rp_dtw_ragged.hip) when every window of
    // the call is scored from LDS-staged tiles (never behind the gate: !gl.count); the averaged template (its own output array) keeps its
    // register launch.  The windows that kernel lists (a frame it cannot resolve within the parity gate: digital silence behind speech, wild
    // scales) are scored again by the register kernels in list mode -- two launches that leave at once when nothing is listed -- or,
    // without slack behind the frame array, by dtw_ref_kernel
    if (!few && !gl.list && !gl.count && t.rag_count > 0 && W <= 5 && c.wk.rag_prep && c.wk.rag_streams >= S &&
        dtw_ragged_supported(t, W, n_win, c.score_ref)) {
        if (t.has_avg && n1 == t.class_count[3] && n1 > 0)
            if ((e = launch_dtw_avg_chunk<5, W>(c, few, gl)) != hipSuccess) return e;
        // (every ragged chunk lists on its own: a window may be listed once per chunk -- the list holds rows x chunks entries)
        const bool list_rows = c.padded_rows && c.wk.rag_list && c.wk.rag_rows >= S * n_win * (size_t)t.rag_count && c.out_win_pitch == n_win;
        if ((e = launch_dtw_ragged(c, gl.abandon_nc, list_rows)) != hipSuccess) return e;
        if (list_rows) {
            GateList g2 = gl;
            g2.list = c.wk.rag_list + 1; g2.count = c.wk.rag_list; g2.dense_min = 0; g2.fuse = nullptr;
            g2.list_mult = (uint32_t)t.rag_count;   // every ragged chunk lists on its own (round-5 advice: a grid for S x n_win entries dropped the tail)
            if ((e = launch_dtw_single_chunks<W>(c, t.class_first[3], t.class_count[3] - (t.has_avg ? 1 : 0), false, g2)) != hipSuccess) return e;
            if ((e = launch_dtw_class<W, 2>(c, t.class_first[0], t.class_count[0], false, g2)) != hipSuccess) return e;
        }
    } else {
        // n1: single-template chunks to score (class 3; the averaged template is its last chunk)
        if ((e = launch_dtw_single_chunks<W>(c, t.class_first[3], n1, few, gl)) != hipSuccess) return e;
        if ((e = launch_dtw_class<W, 2>(c, t.class_first[0], t.class_count[0], few, gl)) != hipSuccess) return e;
    }
    // chunks of 3..8 templates: the matrix-core kernel (rp_dtw_mfma.hip) in every mode (LDS-staged, frames from global memory for
    // live-stream batches and the gate's list, early abandon): 5..8 templates at band 3..5 with eight template slots per wave, 3..4 at
    // band 5 with four.
    {
        const bool from_global = few || gl.list != nullptr;
        if (t.class_count[1] > 0 && dtw_mfma_supported(t, W, n_win, from_global, 4, c.score_ref)) {
            if ((e = launch_dtw_mfma(c, 4, t.class_first[1], t.class_count[1], from_global, gl)) != hipSuccess) return e;
        } else if ((e = launch_dtw_class<W, 4>(c, t.class_first[1], t.class_count[1], few, gl)) != hipSuccess) return e;
        if (t.class_count[2] > 0 && dtw_mfma_supported(t, W, n_win, from_global, 8, c.score_ref)) {
            // several chunks of one length, every window of a long batch scored: the workgroups that share a column's B operand among four
            // (two) chunks (rp_dtw_mfma_group.hip: same bits); the chunks outside a group, and every other mode, keep dtw_mfma_kernel
            // (gl is then no gate, no abandon and no fuse)
            if (!from_global && !gl.count && !gl.fuse && !(gl.abandon_nc < RP_INF) && dtw_mfma_group_supported(t, W, n_win, S, c.score_ref)) {
                if ((e = launch_dtw_mfma_group(c)) != hipSuccess) return e;
                for (int r = 0; r < t.rest_runs; ++r)
                    if ((e = launch_dtw_mfma(c, 8, t.rest_first[r], t.rest_count[r], false, gl)) != hipSuccess) return e;
                return hipSuccess;
            }
            return launch_dtw_mfma(c, 8, t.class_first[2], t.class_count[2], from_global, gl);
        }
    }
    // Small batches: tc-8 waves run two per SIMD; a launch that fills those slots 2.x times leaves the chip mostly idle in
    // its last round.  The same templates as tc-4 half chunks are twice as many waves of 0.83 of the length (measured at C2), three per SIMD
    // (146 VGPRs).  Taken when the modelled makespan is shorter; large batches (>= 3 rounds of tc-8 waves) never are.
    if (t.class_count[2] > 0 && t.split_count == 2 * t.class_count[2] && std::getenv("RP_DTW_NO_SPLIT") == nullptr) {
        const double waves8 = (double)((S * n_win + kDtwWin - 1) / kDtwWin) * t.class_count[2];
        const double slots = 4.0 * device_cu_count();
        const double cost8 = std::ceil(waves8 / (2.0 * slots)), cost4 = 0.85 * std::ceil(2.0 * waves8 / (3.0 * slots));
        if (waves8 < 3.0 * 2.0 * slots && cost4 < cost8) return launch_dtw_class<W, 4>(c, t.split_first, t.split_count, few, gl);
    }
    return launch_dtw_class<W, 8>(c, t.class_first[2], t.class_count[2], few, gl);
}

// ---- the averaged-template gate as a skip (wakeword_comp.rs:85-93) -------------------------------------------------
// The reference scores the window against the averaged template first and returns None when that score is below
// avg_threshold: the T sample templates are never compared.  Batched: pass 1 scores EVERY window against the averaged
// template only, gate_compact_kernel lists the rows that pass, pass 3 runs the sample templates on the listed rows
// (one lane per listed window, frames read from global memory).  Rows that are not listed keep whatever `scores` held.
// One wave lists 16 x 64 consecutive rows with a single atomic (one atomic per wave-row of 64 would serialise on the
// counter: ~300 k atomics at C3); the order inside a wave's block is preserved, so neighbouring windows stay neighbours.
__global__ __launch_bounds__(256) void gate_compact_kernel(const float *__restrict__ avg, size_t rows, float avg_threshold,
                                                           uint32_t *__restrict__ list, uint32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t r0 = wave * 1024;
    if (r0 >= rows) return;
    unsigned long long m[16];
    unsigned total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const size_t r = r0 + (size_t)i * 64 + lane;
        const bool pass = r < rows && !(avg[r] < avg_threshold);  // `avg_score < avg_threshold -> None`
        m[i] = __ballot(pass);
        total += (unsigned)__popcll(m[i]);
    }
    if (total == 0) return;
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(count, total);
    base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if ((m[i] >> lane) & 1ull) list[base + (unsigned)__popcll(m[i] & ((1ull << lane) - 1ull))] = (uint32_t)(r0 + (size_t)i * 64 + lane);
        base += (unsigned)__popcll(m[i]);
    }
}

// ---- the route: which kernels score a call ---------------------------------------------------------------------------
// Decided here once per call, from the template set, the band, the call's shape and whether the averaged template is scored; every
// launcher below reads it.  The callers describe the call (DtwScore, rp_kernels.h) and never pick kernels themselves.
enum DtwGate { kGateNone, kGateRegister, kGateGeneric };
struct DtwRoute {
    // one stream alone is scored like a batch when the matrix-core kernel serves its templates (a stream's bits must not depend on the
    // batch it is scored in, live or offline -- only callers without padded rows, the single-stream mirror, keep dtw_single_kernel)
    bool mfma_batch = false;
    // many streams with few windows each (streaming batches): cross-stream waves reading frames from global memory (needs padded rows:
    // slack after the last stream's frames for the never-used out-of-band columns)
    bool few = false;
    // dtw_single_kernel, one wave per DTW for a handful of windows of one stream: its LDS, whether it takes the set, whether it scores the call
    size_t single_lds = 0;
    bool single_fits = false, single = false;
    // the register kernels (mfcc_size 5: launch_dtw_k5, 13 / 16: launch_dtw_wide_all) score the sample templates; else, unless the set is
    // ref-only (dtw_ref_kernel scores every window), dtw_generic_kernel with generic_lds bytes of LDS
    bool reg = false;
    size_t generic_lds = 0;
    DtwGate gate = kGateNone;   // the averaged-template gate the set supports (padded rows only: its list mode reads past a row)
    bool fuse_max = false;      // ScoreMode::Max can be folded into the matrix-core kernel (DtwFusedAgg)
};

static DtwRoute dtw_route(const TemplatesDev &t, int band, size_t S, size_t n_win, bool padded, bool with_avg, float score_ref) {
    DtwRoute r;
    r.mfma_batch = padded && ((t.K == 5 && ((t.class_count[2] > 0 && dtw_mfma_supported(t, band, n_win, true, 8, score_ref)) ||
                                            (t.class_count[1] > 0 && dtw_mfma_supported(t, band, n_win, true, 4, score_ref)))) ||
                              dtw_mfma_wide_supported(t, band, score_ref) || dtw_mfma_wide3_supported(t, band));
    r.few = padded && (S > 1 || r.mfma_batch) && n_win < (size_t)kDtwWin;
    if (S == 1 && n_win <= 8 && t.max_diff == 0 && band >= 1 && 2 * band <= 16) {
        r.single_lds = (2 * (size_t)t.max_len * (t.K | 1) + ((t.K + 3) & ~3) + (size_t)(2 * t.max_len + 2 * band + 16) * 2 * band) * sizeof(float);
        r.single_fits = r.single_lds <= 64 * 1024;
    }
    r.single = r.single_fits && !r.mfma_batch;
    // the register kernels assume m == n (no template longer than the window)
    // (a register kernel stages 64..128 windows + two template lengths of frames in LDS: templates beyond ~4 000 frames at
    // mfcc_size 5 -- 40 s -- do not fit the CU's 160 KB; the generic kernel stages one length and takes them up to ~8 000)
    const bool reg_built = dtw_register_tile(t.K, band) > 0 && t.max_diff == 0 && t.chunks;
    static_assert(kDtwWin == 64, "dtw_register_staged");
    const bool reg_staged = reg_built && dtw_register_staged(t.K, t.max_len);
    // (a window past the staging goes to dtw_generic_kernel whatever the call's shape, also where `few` would let the register kernels read
    // it from global memory: which frames a window's norm-range test sees -- the register kernels' include the W - 2 loaded behind its end,
    // the generic kernel's do not -- then depends on the template set alone, and a wakeword bank can follow it: BankWakeword::window_chk)
    r.reg = !r.single && !t.ref_only && reg_built && reg_staged;
    // the band is widened to |m-n| inside the generic kernel; size for the worst case over templates
    const int KP = t.K | 1, Wmax = band > t.max_diff ? band : t.max_diff;
    r.generic_lds = ((size_t)(64 + t.max_len - 1) * KP + (size_t)t.K * 64 + (size_t)(2 * Wmax + 1) * 64) * sizeof(float);
    const size_t rows = S * n_win;
    if (padded && t.has_avg && rows > 0) {
        if (!t.ref_only && reg_staged && rows < 0xffffffffULL) r.gate = kGateRegister;
        else if (!r.single_fits && (t.ref_only || !reg_staged)) r.gate = kGateGeneric;
    }
    // ScoreMode::Max inside the matrix-core kernel: one chunk of 3..8 templates is all there is to score
    const int n2 = t.class_count[3] - ((t.has_avg && !with_avg) ? 1 : 0);   // single-template chunks to score
    r.fuse_max = r.reg && t.K == 5 && n2 == 0 && t.class_count[0] == 0 && t.class_count[1] + t.class_count[2] == 1 && band >= 3 && band <= 5 &&
                 std::getenv("RP_DTW_NO_FUSED_MAX") == nullptr && dtw_mfma_supported(t, band, n_win, r.few, t.class_count[2] == 1 ? 8 : 4, score_ref);
    return r;
}

// e = CALL(K, W) on the (mfcc_size, band) pairs the register kernels are built for (dtw_register_tile > 0).  (A switch, not a generic
// lambda: it keeps the order in which the kernel templates are instantiated, and with it the layout of the code object.)
#define RP_BAND_DISPATCH(e, CALL, KK) \
    switch (c.band) { case 3: e = CALL(KK, 3); break; case 4: e = CALL(KK, 4); break; case 5: e = CALL(KK, 5); break; default: e = CALL(KK, 6); }

// The register family of the call's (mfcc_size, band): the averaged template's chunk alone (AVG_ONLY), or n1 single-template chunks and
// then the chunks of several templates.  (AVG_ONLY is a template parameter for the same reason as the switch: the gate names <true>
// first, so every one-template kernel is still instantiated before the others.)
template <bool AVG_ONLY, int K, int W>
static hipError_t launch_dtw_register_kw(const DtwCall &c, int n1, bool few, const GateList &gl) {
    if constexpr (AVG_ONLY) return launch_dtw_avg_chunk<K, W>(c, few, gl);
    else if constexpr (K == 5) return launch_dtw_k5<W>(c, n1, few, gl);
    else return launch_dtw_wide_all<K, W>(c, n1, few, gl);
}
template <bool AVG_ONLY>
static hipError_t launch_dtw_register(const DtwCall &c, int n1, bool few, const GateList &gl) {
    hipError_t e;
#define RP_REGISTER(KK, WW) launch_dtw_register_kw<AVG_ONLY, KK, WW>(c, n1, few, gl)
    if (c.t->K == 5) { RP_BAND_DISPATCH(e, RP_REGISTER, 5) } else if (c.t->K == 16) { RP_BAND_DISPATCH(e, RP_REGISTER, 16) } else { RP_BAND_DISPATCH(e, RP_REGISTER, 13) }
#undef RP_REGISTER
    return e;
}

// The gate behind the register kernels (few: DtwRoute::few -- live-stream batches score the few newest windows of every stream: then
// pass 1 also reads its frames from global memory); list [1 + S * n_win] words, the first the count.
static hipError_t gated_register(const DtwCall &c, bool few, float avg_threshold, uint32_t *list, float abandon_nc) {
    const TemplatesDev &t = *c.t;
    const size_t rows = c.S * c.n_win;
    hipError_t e;
    if ((e = hipMemsetAsync(list, 0, sizeof(uint32_t), c.st)) != hipSuccess) return e;
    // pass 1: the averaged template over every window (and, before the gate looks at them, the reference-shaped rescoring of the
    // windows whose frames left the norm range: dtw_ref_kernel)
    if ((e = launch_dtw_register<true>(c, 0, few, GateList{})) != hipSuccess) return e;
    if ((e = launch_dtw_ref(c, false, t.T, 1)) != hipSuccess) return e;
    // pass 2: list the rows whose avg_score is not below the threshold
    const size_t waves = (rows + 1023) / 1024, blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(gate_compact_kernel, dim3((unsigned)blocks), dim3(256), 0, c.st, c.avg, rows, avg_threshold, list + 1, list);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // pass 3: the sample templates on the listed rows -- or, when (nearly) every row is listed, on all rows through the
    // ordinary staged launch (GateList; with few windows per stream both forms read global memory: list mode only)
    GateList gl;
    gl.list = list + 1; gl.count = list; gl.abandon_nc = abandon_nc;
    gl.dense_min = few ? 0u : (uint32_t)(rows - rows / 10);
    if ((e = launch_dtw_register<false>(c, t.class_count[3] - 1, false, gl)) != hipSuccess) return e;
    if (!few) {
        gl.list = nullptr;
        if ((e = launch_dtw_register<false>(c, t.class_count[3] - 1, false, gl)) != hipSuccess) return e;
    }
    return launch_dtw_ref(c, false, 0, t.T);
}

// dtw_generic_kernel over templates t_first .. t_first + t_count - 1 (index T = the averaged template); gate_avg: each wave leaves at once
// when none of its 64 windows has gate_avg[row] >= gate_threshold
static hipError_t launch_dtw_generic(const DtwCall &c, const DtwRoute &r, int t_first, int t_count, const float *gate_avg, float gate_threshold) {
    const TemplatesDev &t = *c.t;
    const size_t tiles = (c.n_win + kDtwWin - 1) / kDtwWin, blocks = tiles * (size_t)t_count * c.S;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    if (r.generic_lds > 160 * 1024) return hipErrorMemoryAllocation;  // reported as "template too long" by the callers' hip_ok text
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(dtw_generic_kernel), 160 * 1024); e != hipSuccess) return e;
    hipLaunchKernelGGL(dtw_generic_kernel, dim3((unsigned)blocks), dim3(64), r.generic_lds, c.st, c.mfcc, c.frame_pitch, c.frame_pitch, (unsigned)tiles,
                       c.first_win, c.n_win, c.out_win_pitch, t.lens, t.unit, t.Lpad, t.K, t.T, t_first, t_count, t.max_len, c.band, c.score_ref,
                       c.scores, c.avg, gate_avg, gate_threshold, c.wk.fix);
    return hipGetLastError();
}

// The gate behind the generic kernel: pass 1 scores every window against the averaged template (-> avg), pass 2 the sample
// templates, each wave leaving at once when none of its 64 windows passed (scores of such rows are not written; the aggregate
// pass gives them 0).
static hipError_t gated_generic(const DtwCall &c, const DtwRoute &r, float avg_threshold) {
    const TemplatesDev &t = *c.t;
    hipError_t e;
    if (t.ref_only) {  // a template row outside the norm range: every window reference-shaped, no skipping (the aggregate pass writes 0 for rejected rows)
        if ((e = launch_dtw_ref(c, true, t.T, 1)) != hipSuccess) return e;
        return launch_dtw_ref(c, true, 0, t.T);
    }
    if ((e = launch_dtw_generic(c, r, t.T, 1, nullptr, 0.f)) != hipSuccess) return e;
    // the gate must see reference-shaped avg scores: rescoring of the listed windows first
    if ((e = launch_dtw_ref(c, false, t.T, 1)) != hipSuccess) return e;
    if ((e = launch_dtw_generic(c, r, 0, t.T, c.avg, avg_threshold)) != hipSuccess) return e;
    return launch_dtw_ref(c, false, 0, t.T);
}

// The averaged-template gate in the form the route names (r.gate != kGateNone)
static hipError_t launch_dtw_gated(const DtwCall &c, const DtwRoute &r, float avg_threshold, uint32_t *list, float abandon_nc) {
    const hipError_t e = r.gate == kGateGeneric ? gated_generic(c, r, avg_threshold) : gated_register(c, r.few, avg_threshold, list, abandon_nc);
    return e == hipSuccess ? e : dtw_abort(c.st, c.wk, e);
}

// Normalised-cost bound above which a DTW cannot reach `threshold` any more: score = 1 / (1 + exp((nc - ref) / ref)) > thr
// <=> nc < ref * (1 + ln(1/thr - 1)) (comparator.rs:18-26), with a margin for the rounding of the running costs.
static float dtw_abandon_nc(float threshold, float score_ref) {
    if (!(score_ref > 0.f) || !(threshold > 0.f)) return __builtin_inff();  // everything can fire (or the formula is degenerate): never abandon
    if (threshold >= 1.f) return 0.f;                                         // a score is < 1: nothing can fire
    const float nc = score_ref * (1.f + logf(1.f / threshold - 1.f));
    return nc > 0.f ? nc * 1.001f + 1e-4f : nc + 1e-4f;
}

// The ungated fast launches: dtw_single_kernel, the register kernels or dtw_generic_kernel.  fuse: the caller's ScoreMode::Max outputs;
// `done` is set when the matrix-core kernel writes them.
static hipError_t launch_dtw_fast(const DtwCall &c, const DtwRoute &r, int Ttot, float abandon_nc, DtwFusedAgg *fuse) {
    const TemplatesDev &t = *c.t;
    if (r.single) {
        dtw_mark(c.wk, kDtwRanSingle);
        return launch_dtw_single(c, r.single_lds, 0, Ttot);
    }
    if (r.reg) {
        GateList gl;
        gl.abandon_nc = abandon_nc;
        if (fuse && fuse->agg && r.fuse_max) {
            gl.fuse = fuse;
            fuse->done = true;
        }
        // single-template chunks to score: the averaged template is the last of them, scored when Ttot counts it
        return launch_dtw_register<false>(c, t.class_count[3] - ((t.has_avg && Ttot == t.T) ? 1 : 0), r.few, gl);
    }
    const hipError_t e = launch_dtw_generic(c, r, 0, Ttot, nullptr, 0.f);
    if (e == hipSuccess) dtw_mark(c.wk, kDtwRanGeneric);
    return e;
}

// The ungated call: the fast launches, then dtw_ref_kernel's pass over the windows they listed (a frame outside the norm range) -- or
// over every window for a template set with such a row.
static hipError_t launch_dtw(const DtwCall &c, const DtwRoute &r, bool with_avg, float abandon_nc, DtwFusedAgg *fuse) {
    const TemplatesDev &t = *c.t;
    if (fuse) fuse->done = false;
    if (c.S == 0 || c.n_win == 0) return hipSuccess;
    if (!c.wk.fix || !c.wk.sched) return hipErrorInvalidValue;
    if (t.n_chunks_total > kDtwSchedChunks) return hipErrorInvalidValue;
    const int Ttot = t.T + ((with_avg && t.has_avg) ? 1 : 0);
    if (r.single || !t.ref_only) {   // (dtw_single_kernel takes a ref-only set itself)
        if (hipError_t e = launch_dtw_fast(c, r, Ttot, abandon_nc, fuse); e != hipSuccess) return dtw_abort(c.st, c.wk, e);
        if (r.single) return hipSuccess;
    }
    const hipError_t e = launch_dtw_ref(c, t.ref_only != 0, 0, Ttot, (fuse && fuse->done) ? fuse : nullptr);
    return e == hipSuccess ? e : dtw_abort(c.st, c.wk, e);
}

// A handful of windows of ONE stream (the single-stream API), templates t_first .. t_first + t_count - 1 only (index T = the
// averaged template): the caller scores the averaged template first and the sample templates only when a window passed
// the gate.  hipErrorNotSupported when dtw_single_kernel does not take this set (the caller then scores everything).
hipError_t launch_dtw_single_part(hipStream_t st, const DtwWork &wk, const TemplatesDev &t, const float *mfcc, size_t frame_pitch, size_t first_win, size_t n_win,
                                  size_t out_win_pitch, int band, float score_ref, int t_first, int t_count, float *scores, float *avg) {
    if (n_win == 0 || t_count <= 0) return hipSuccess;
    const DtwRoute r = dtw_route(t, band, 1, n_win, false, true, score_ref);
    if (!r.single_fits || t_first + t_count > t.T + (t.has_avg ? 1 : 0)) return hipErrorNotSupported;
    DtwCall c;
    c.st = st; c.wk = wk; c.t = &t; c.mfcc = mfcc; c.S = 1; c.frame_pitch = frame_pitch; c.first_win = first_win; c.n_win = n_win;
    c.out_win_pitch = out_win_pitch; c.band = band; c.score_ref = score_ref; c.scores = scores; c.avg = avg;
    return launch_dtw_single(c, r.single_lds, t_first, t_count);
}

// -------------------------------------------------------------------- aggregate
// src/wakewords/comp/wakeword_comp.rs:38-49 (get_percentile) and :108-139
// (percentile_sorted and percentile_of_mode: rp_device.h, shared with dtw_bank_kernel)

bool aggregate_fits(int T) {
    if (T <= kAggMaxT) return true;
    set_last_error("a wakeword reference of " + std::to_string(T) + " templates exceeds the " + std::to_string(kAggMaxT) +
                   "-template limit of the score aggregate");
    return false;
}

// Max / Average: no sort buffer, so no scratch memory to set up (the single-stream path launches this for 3 rows).
// A workgroup owns 64 consecutive rows: the [64][T] block of scores is one contiguous range, copied to LDS with
// coalesced loads (row pitch T+1: conflict-free), then lane r walks row r in template order.
// What a row's aggregate means downstream: a window the averaged-template gate rejected was never compared with the
// sample templates (its `scores` row holds nothing), so its aggregate is written as 0 here instead of leaving that to the
// scan's own avg test; and the first window of a stream that can fire (agg > threshold, gate passed) raises the stream's
// `hot` flag, so that scan_kernel does not have to sweep the rows of quiet streams to learn that nothing can happen
// (src/detector.rs:398-430: without such a window no partial detection ever exists).
__device__ __forceinline__ void agg_store(float *__restrict__ agg, size_t row, float a, const AggExtra &x) {
    const bool gated = x.gate_avg && x.gate_avg[row] < x.gate_threshold;
    if (gated) a = 0.f;
    agg[row] = a;
    if (x.hot && !gated && a > x.threshold) x.hot[row / x.n_win] = 1u;   // every writer stores the same value
}

__global__ __launch_bounds__(64) void aggregate_kernel(const float *__restrict__ scores, size_t n_rows, int T, int mode,
                                                       float *__restrict__ agg, AggExtra x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tile = reinterpret_cast<float *>(smem);  // [64][T + 1]
    const size_t row0 = (size_t)blockIdx.x * 64;
    const size_t nr = n_rows - row0 < 64 ? n_rows - row0 : 64;
    const float *src = scores + row0 * T;
    const int total = (int)nr * T, P = T + 1;
    for (int i = threadIdx.x; i < total; i += 64) {
        const int r = i / T, t = i - r * T;
        tile[r * P + t] = src[i];
    }
    __syncthreads();
    const int r = threadIdx.x;
    if ((size_t)r >= nr) return;
    const float *v = tile + r * P;
    if (mode == 1) {  // Max
        float m = v[0];
        for (int i = 1; i < T; ++i) m = fmaxf(m, v[i]);
        agg_store(agg, row0 + r, m, x);
    } else {  // Average: sequential sum in template order
        float sum = 0.f;
        for (int i = 0; i < T; ++i) sum += v[i];
        agg_store(agg, row0 + r, sum / (float)T, x);
    }
}

// Median / percentiles: sort ascending, then the reference's f32 interpolation (wakeword_comp.rs:38-49).
// T <= 64: a workgroup copies its 64 rows [64][T] (one contiguous block) to LDS with coalesced loads, lane r takes row r
// into NT registers (padded with +inf) and sorts them with a compile-time bitonic network -- no scratch memory, no
// data-dependent loop; the percentile position depends only on T and the mode, so it is wave-uniform.
template <int NT> __device__ __forceinline__ void bitonic_sort(float (&v)[NT]) {
#pragma unroll
    for (int k = 2; k <= NT; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const float a = v[i], b = v[l];
                    const float lo = fminf(a, b), hi = fmaxf(a, b);
                    v[i] = up ? lo : hi;
                    v[l] = up ? hi : lo;
                }
            }
}

template <int NT>
__global__ __launch_bounds__(64) void aggregate_sorted_reg_kernel(const float *__restrict__ scores, size_t n_rows, int T, int mode,
                                                                  float *__restrict__ agg, AggExtra x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tile = reinterpret_cast<float *>(smem);  // [64][T + 1]
    const size_t row0 = (size_t)blockIdx.x * 64;
    const size_t nr = n_rows - row0 < 64 ? n_rows - row0 : 64;
    const float *src = scores + row0 * T;
    const int total = (int)nr * T, P = T + 1;
    for (int i = threadIdx.x; i < total; i += 64) {
        const int r = i / T, t = i - r * T;
        tile[r * P + t] = src[i];
    }
    __syncthreads();
    const int r = threadIdx.x;
    if ((size_t)r >= nr) return;
    float v[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) v[i] = i < T ? tile[r * P + i] : RP_INF;
    bitonic_sort<NT>(v);
    // get_percentile: index = p/100 * (T-1) in f32; an exact integer takes the element, else linear interpolation
    const float index = percentile_of_mode(mode) / 100.0f * (float)(T - 1);
    const float fl = floorf(index);
    const int i0 = (int)fl;  // wave-uniform
    float lo = 0.f, hi = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        lo = i == i0 ? v[i] : lo;
        hi = i == i0 + 1 ? v[i] : hi;
    }
    const float d = index - fl;
    agg_store(agg, row0 + r, fl == index ? lo : lo * (1.0f - d) + hi * d, x);
}

// T > 64: per-lane insertion sort in scratch memory
__global__ __launch_bounds__(64) void aggregate_sorted_kernel(const float *__restrict__ scores, size_t n_rows, int T, int mode,
                                                              float *__restrict__ agg, AggExtra x) {
    size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= n_rows) return;
    const float *v = scores + row * T;
    float tmp[kAggMaxT];
    for (int i = 0; i < T; ++i) {  // insertion sort ascending (total_cmp order for non-NaN scores)
        float x = v[i];
        int j = i - 1;
        while (j >= 0 && tmp[j] > x) { tmp[j + 1] = tmp[j]; --j; }
        tmp[j + 1] = x;
    }
    agg_store(agg, row, percentile_sorted(tmp, T, percentile_of_mode(mode)), x);
}

hipError_t launch_aggregate(hipStream_t st, const float *scores, size_t n_rows, int T, int mode, float *agg, AggExtra x) {
    if (n_rows == 0) return hipSuccess;
    if (T < 1 || T > kAggMaxT) return hipErrorInvalidValue;
    size_t blocks = (n_rows + 63) / 64;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    if (mode == 0 || mode == 1) {
        // T = 256 asks for 65 792 bytes.  The runtime on gfx950 bounds a launch by the device's 160 KB per workgroup and ran it unasked
        // (tests/test_gpu_aggregate_builds.py at 256 templates); the opt-in HIP documents above 64 KB is made anyway, as for every other
        // kernel of the library that can pass it
        const size_t lds = (size_t)64 * (T + 1) * sizeof(float);
        if (lds > 64 * 1024)
            if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(aggregate_kernel), 160 * 1024); e != hipSuccess) return e;
        hipLaunchKernelGGL(aggregate_kernel, dim3((unsigned)blocks), dim3(64), lds, st, scores, n_rows, T, mode, agg, x);
    } else if (T <= 64) {
        const size_t lds = (size_t)64 * (T + 1) * sizeof(float);
#define RP_AGG_SORTED(NT) hipLaunchKernelGGL(aggregate_sorted_reg_kernel<NT>, dim3((unsigned)blocks), dim3(64), lds, st, scores, n_rows, T, mode, agg, x)
        if (T <= 2) RP_AGG_SORTED(2);
        else if (T <= 4) RP_AGG_SORTED(4);
        else if (T <= 8) RP_AGG_SORTED(8);
        else if (T <= 16) RP_AGG_SORTED(16);
        else if (T <= 32) RP_AGG_SORTED(32);
        else RP_AGG_SORTED(64);
#undef RP_AGG_SORTED
    } else hipLaunchKernelGGL(aggregate_sorted_kernel, dim3((unsigned)blocks), dim3(64), 0, st, scores, n_rows, T, mode, agg, x);
    return hipGetLastError();
}


// -------------------------------------------------------------------- one scoring call: DTW, then aggregate
bool dtw_score(Ctx &c, const DtwScore &q) {
    const TemplatesDev &t = *q.t;
    const size_t rows = q.S * q.n_win;
    if (q.agg && !aggregate_fits(t.T)) return false;
    const DtwRoute r = dtw_route(t, q.band, q.S, q.n_win, q.padded_rows, q.with_avg, q.score_ref);
    // The averaged-template gate as the reference runs it (wakeword_comp.rs:85-93): a window whose avg_score is below avg_threshold is
    // never compared with the sample templates
    const bool gated = q.with_avg && q.detect_only && (r.gate == kGateRegister || (r.gate == kGateGeneric && q.gate_generic)) &&
                       (q.gate_one_stream || !(q.S == 1 && q.n_win <= 8));
    // detect-only calls in ScoreMode::Max may also stop DTWs that can no longer reach `threshold` (GateList::abandon_nc)
    const float abandon = (q.detect_only && q.score_mode == RP_SCORE_MAX) ? dtw_abandon_nc(q.threshold, q.score_ref) : __builtin_inff();
    uint32_t *list = q.gate_list;
    if (gated && !list) {
        if (!c.ws_list.reserve((rows + 1) * sizeof(uint32_t) + 16)) return false;
        list = c.ws_list.as<uint32_t>();
    }
    // ScoreMode::Max of a reference whose templates are one chunk of the matrix-core kernel, no averaged template scored: the DTW
    // kernel writes the aggregate (and the flags) itself and the aggregate pass is skipped
    DtwFusedAgg fz;
    if (q.fuse_max && q.score_mode == RP_SCORE_MAX && !q.with_avg && rows && q.agg) { fz.agg = q.agg; fz.hot = q.hot; fz.threshold = q.threshold; }
    // (dtw_ragged_kernel's blocks are reserved for the ungated launch only)
    DtwCall call;
    call.st = c.stream;
    call.wk = (q.ragged && !gated) ? c.dtw_work_for(q.S, rows * (size_t)(t.rag_count > 1 ? t.rag_count : 1)) : c.dtw_work();
    call.t = &t; call.mfcc = q.mfcc; call.S = q.S; call.frame_pitch = q.frame_pitch; call.first_win = q.first_win; call.n_win = q.n_win;
    call.out_win_pitch = q.n_win; call.band = q.band; call.score_ref = q.score_ref; call.scores = q.scores; call.avg = q.avg;
    call.padded_rows = q.padded_rows;
    if (q.timed) c.time_begin(kKernelDtw);
    bool ok = gated ? hip_ok(launch_dtw_gated(call, r, q.avg_threshold, list, abandon), r.gate == kGateRegister ? "dtw kernels (gated)" : "dtw_generic_kernel (gated)")
                    : hip_ok(launch_dtw(call, r, q.with_avg, abandon, fz.agg ? &fz : nullptr), "dtw kernel");
    if (q.timed) c.time_end();
    if (!ok || !q.agg || fz.done) return ok;
    // the aggregate pass: 0 for the windows the gate rejected (their `scores` rows were never written) and, with `hot`, the flags
    // that tell the scan which streams can fire at all
    AggExtra ax;
    if (q.hot) { ax.hot = q.hot; ax.threshold = q.threshold; ax.n_win = q.n_win; }
    if (gated) { ax.gate_avg = q.avg; ax.gate_threshold = q.avg_threshold; }
    if (q.timed) c.time_begin(kKernelAggregate);
    ok = hip_ok(launch_aggregate(c.stream, q.scores, rows, t.T, q.score_mode, q.agg, ax), "aggregate_kernel");
    if (q.timed) c.time_end();
    return ok;
}

}  // namespace rp
