// rp_dtw_set.hip -- window scoring where stream s carries a SET of wakewords of a bank, bank[stream_wakewords[s][0 .. set_size)] (-1: an empty
// slot) -- the batched form of one `Rustpotter` per user with several add_wakeword calls (src/detector.rs:304-346,433-447).  The window is as
// long as the longest wakeword of the stream's set, Lmax(s), and every wakeword scores its oldest frames (wakeword_comp.rs:22-27).
// dtw_set_kernel: whole recordings, one wave per (stream, tile of 64 window starts), the slots walked by the wave and the window's proposal
// folded in registers; dtw_set_stream_kernel: the new windows of a live-stream batch, lanes = rows of [S][set_size][n_new], and
// dtw_mixed_stream_kernel, the same for a stream that also holds models (Lmax(s) over both).  The DTW walks
// are those of rp_dtw_bank.hip (rp_dtw_bank.h), operation for operation.  DESIGN.md §4.2c.
#include "rp_device.h"
#include "rp_dtw_bank.h"

namespace rp {

// One wave = one (stream, tile of 64 consecutive window starts); lane = window.  The tile's 64 + Lmax(s) + W frames are staged in LDS once;
// the wave then walks the slots of its stream's set and, per slot, that wakeword exactly as dtw_bank_kernel walks its one: the averaged
// template first when it is to be scored, the gate at wave granularity, the score_mode aggregate folded as it goes, the norm-range test and
// the reference-shaped rescoring, the percentile block (reused slot after slot: a lane only ever reads its own column).  A window of the
// set starts where the bank call's window of that wakeword starts, so slot (s, j) gets the bits rp_dtw_score_bank gives wakeword set[s][j]
// for the first n_win_s = n_frames - Lmax(s) + 1 window starts.
// The set row and everything read through it are wave-uniform: scalar loads.  (The bank's arrays and the call's are separate __restrict__
// parameters for the reason dtw_bank_kernel gives.)
// Written: the window's proposal (run_wakeword_detectors, src/detector.rs:433-447) as three rows [S][win_pitch] -- the best passing
// aggregate, its averaged-template score and its BANK index, -1 where no wakeword proposes; the first slot of equals wins -- when best_ww is
// given, hot[s] for a stream with a proposal, and the per-slot rows [S][set_size][win_pitch] only when slot_agg is given: detection needs
// the three rows alone, a set_size-th of the memory.
template <int K, int W>
__global__ __launch_bounds__(64) void dtw_set_kernel(const BankWakeword *__restrict__ bank_ww, const int *__restrict__ bank_tlen,
                                                     const long long *__restrict__ bank_trow, const float *__restrict__ bank_unit,
                                                     const float *__restrict__ bank_raw, const float *__restrict__ mfcc,
                                                     const int32_t *__restrict__ stream_wakewords, float *__restrict__ best,
                                                     float *__restrict__ best_avg, int32_t *__restrict__ best_ww, float *__restrict__ slot_agg,
                                                     float *__restrict__ slot_avg, uint32_t *__restrict__ hot, uint32_t *__restrict__ fix,
                                                     BankDev b, BankSetScore q, unsigned tiles) {
    constexpr int KP = (K % 2 == 0) ? K + 1 : K;  // odd pitch: conflict-free lane-strided LDS reads
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);               // [64 + b.max_len + 6][KP]
    float *sl = xs + (size_t)(64 + b.max_len + 6) * KP;        // [kBankMaxTemplates][64]: a lane's scores (percentile modes)
    float *Pb = sl + kBankMaxTemplates * 64;                   // [13][64]: band of the reference-shaped cell

    const unsigned tile = blockIdx.x % tiles;
    const size_t s = blockIdx.x / tiles;
    const int lane = threadIdx.x;
    const size_t wl = (size_t)tile * 64 + lane;
    const int32_t *set = stream_wakewords + s * (size_t)q.set_size;
    // on_wakeword_change, src/detector.rs:328-334: the longest wakeword of the detector sets the window
    int lmax = 0;
    for (int j = 0; j < q.set_size; ++j) {
        const int wi = set[j];
        if (wi >= 0 && wi < b.W) lmax = max(lmax, bank_ww[wi].max_len);   // an index outside the bank is an empty slot here
    }
    const size_t n_win = (lmax > 0 && q.n_frames >= (size_t)lmax) ? q.n_frames - (size_t)lmax + 1 : 0;
    const bool in_row = wl < q.win_pitch;
    const bool tile_empty = (size_t)tile * 64 >= n_win;
    if (!tile_empty) {
        const int n_stage = 64 + lmax + W;
        const float *src = mfcc + s * q.n_frames * K;
        const size_t w0 = (size_t)tile * 64;
        for (int i = lane; i < n_stage * K; i += 64) {
            const int f = i / K, k = i - f * K;
            const size_t g = w0 + f;
            xs[f * KP + k] = g < q.n_frames ? src[g * K + k] : 0.f;
        }
        __syncthreads();
    }
    const float *xl = xs + lane * KP;
    const bool valid = wl < n_win;
    const int mode = q.score_mode;
    float p_score = 0.f, p_avg = 0.f;
    int p_ww = -1;
    for (int j = 0; j < q.set_size; ++j) {
        const int wi = set[j];
        float a = 0.f, avg_sc = 0.f;
        bool do_avg = false;
        if (!tile_empty && wi >= 0 && wi < b.W) {   // wave-uniform
            const BankWakeword *bw = bank_ww + wi;
            const float own_thr = bw->threshold, own_athr = bw->avg_threshold;
            const float thr = own_thr == own_thr ? own_thr : q.threshold;
            const float athr = own_athr == own_athr ? own_athr : q.avg_threshold;
            const int avg_e = bw->avg, T = bw->count, first = bw->first, ref_only = bw->ref_only, window_chk = bw->window_chk;
            do_avg = avg_e >= 0 && (q.avg_mode == 1 || (q.avg_mode == 2 && athr != 0.f));   // wakeword_comp.rs:85
            float acc = 0.f;
            bool scored = true;
            for (int ti = do_avg ? -1 : 0; ti < T; ++ti) {
                const int e = ti < 0 ? avg_e : first + ti;
                const int L = bank_tlen[e];
                const size_t off = (size_t)bank_trow[e] * K;
                float chk;
                float sc = bank_dtw<K, W, KP>(xl, L, bank_unit + off, q.score_ref, chk);
                if (window_chk && __any(valid && chk > kDtwFixLimit)) chk = bank_chk_window<K, KP>(xl, L);   // wave-uniform
                const bool slow = valid && (ref_only || chk > kDtwFixLimit);
                const unsigned long long slow_mask = __ballot(slow);
                if (slow_mask) {   // wave-uniform
                    const float rs = bank_dtw_ref<K, W, KP>(xl, L, bank_raw + off, q.score_ref, Pb, lane);
                    if (slow) sc = rs;
                    if (lane == 0 && fix) atomicAdd(dtw_fix_stats(fix), (unsigned long long)__popcll(slow_mask));   // rp_ctx_dtw_ref_pairs
                }
                if (ti < 0) {
                    avg_sc = sc;
                    // the averaged-template gate (wakeword_comp.rs:85-93) at wave granularity, as dtw_bank_kernel
                    if (q.gate && !__any(valid && !(sc < athr))) { scored = false; break; }
                } else if (mode == 1) acc = ti == 0 ? sc : fmaxf(acc, sc);   // Max
                else if (mode == 0) acc += sc;                               // Average: sequential sum in template order
                else sl[ti * 64 + lane] = sc;
            }
            if (scored) {
                if (mode == 1) a = acc;
                else if (mode == 0) a = acc / (float)T;
                else {   // Median / percentiles: the lane sorts its column ascending, then the reference's f32 interpolation
                    for (int i = 1; i < T; ++i) {
                        const float x = sl[i * 64 + lane];
                        int p = i - 1;
                        while (p >= 0 && sl[p * 64 + lane] > x) { sl[(p + 1) * 64 + lane] = sl[p * 64 + lane]; --p; }
                        sl[(p + 1) * 64 + lane] = x;
                    }
                    a = percentile_sorted(sl + lane, T, percentile_of_mode(mode), 64);
                }
            }
            // agg_store's rules (rp_dtw.hip): a window the gate rejected was never compared -> aggregate 0
            const bool gated = q.gate && do_avg && avg_sc < athr;
            if (gated) a = 0.f;
            if (!valid) { a = 0.f; avg_sc = 0.f; }
            if (!do_avg) avg_sc = 0.f;
            // this wakeword's proposal for the window: its own thresholds, the avg test only where it was scored (propose_one's rule)
            const bool pass = valid && !(do_avg && avg_sc < athr) && a > thr;
            if (pass && (p_ww < 0 || a > p_score)) { p_ww = wi; p_score = a; p_avg = avg_sc; }
        }
        if (slot_agg && in_row) {
            const size_t at = (s * (size_t)q.set_size + j) * q.win_pitch + wl;
            slot_agg[at] = a;
            if (slot_avg) slot_avg[at] = avg_sc;
        }
    }
    if (best_ww && in_row) {
        const size_t at = s * q.win_pitch + wl;
        best[at] = p_score;
        best_avg[at] = p_avg;
        best_ww[at] = p_ww;
    }
    if (hot && __any(p_ww >= 0) && lane == 0) hot[s] = 1u;
}

template <int K, int W>
static hipError_t launch_set_kw(hipStream_t st, const BankDev &b, const BankSetScore &q, unsigned blocks, unsigned tiles, size_t lds) {
    const auto kernel = dtw_set_kernel<K, W>;
    if (lds > 64 * 1024)
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), 160 * 1024); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, st, b.ww, b.tlen, b.trow, b.unit, b.raw, q.mfcc, q.stream_wakewords, q.best, q.best_avg,
                       q.best_ww, q.slot_agg, q.slot_avg, q.hot, q.fix, b, q, tiles);
    return hipGetLastError();
}

hipError_t launch_dtw_set(hipStream_t st, const BankDev &b, const BankSetScore &q) {
    if (q.S == 0 || q.win_pitch == 0) return hipSuccess;
    if (q.set_size < 1 || q.set_size > kScanMaxWakewords || (q.best_ww && (!q.best || !q.best_avg))) return hipErrorInvalidValue;
    if (dtw_register_tile(b.K, q.band) <= 0) return hipErrorNotSupported;
    const size_t tiles = (q.win_pitch + 63) / 64, blocks = tiles * q.S;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = dtw_bank_lds_bytes(b.K, b.max_len);
    if (lds > 160 * 1024) return hipErrorMemoryAllocation;
#define RP_SET(KK, WW) launch_set_kw<KK, WW>(st, b, q, (unsigned)blocks, (unsigned)tiles, lds)
#define RP_SET_BAND(KK) \
    switch (q.band) { case 3: return RP_SET(KK, 3); case 4: return RP_SET(KK, 4); case 5: return RP_SET(KK, 5); default: return RP_SET(KK, 6); }
    if (b.K == 5) { RP_SET_BAND(5) }
    if (b.K == 13) { RP_SET_BAND(13) }
    RP_SET_BAND(16)
#undef RP_SET_BAND
#undef RP_SET
}

// dtw_set_kernel for a live-stream batch (rp_stream_batch_new_bank_sets).  A call brings few windows, so slots are rows: the wave's 64 lanes
// are consecutive rows of the flattened [S][set_size][n_new] space, windows minor, so that neighbouring lanes mostly share a wakeword.  Every
// lane does what a lane of dtw_bank_stream_kernel does for the wakeword of its slot, set[s][j] -- its own template walk, the per-lane gate,
// norm-range test, reference-shaped rescoring and percentile block as there -- except that its window starts Lmax(s) - 1 frames before new
// frame i, Lmax(s) the longest window of the stream's set, read from the bank in every call.  agg / avg [S][set_size][n_new]; an empty slot
// gets zero rows.
template <int K, int W>
__global__ __launch_bounds__(64) void dtw_set_stream_kernel(const BankWakeword *__restrict__ bank_ww, const int *__restrict__ bank_tlen,
                                                            const long long *__restrict__ bank_trow, const float *__restrict__ bank_unit,
                                                            const float *__restrict__ bank_raw, const float *__restrict__ mfcc,
                                                            const int32_t *__restrict__ stream_wakewords, float *__restrict__ agg,
                                                            float *__restrict__ avg, uint32_t *__restrict__ fix, int bank_W, int set_size,
                                                            BankStreamScore q) {
    __shared__ float sl[kBankMaxTemplates * 64];   // a lane's scores (percentile modes), lane-minor
    __shared__ float Pb[13 * 64];                  // band of the reference-shaped cell
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x * 64u + lane, n_new = (uint32_t)q.n_new;
    const bool valid = row < (uint32_t)(q.S * (size_t)set_size * q.n_new);
    const uint32_t sj = valid ? row / n_new : 0u, i = row - sj * n_new;   // sj = s * set_size + j
    const uint32_t s = sj / (uint32_t)set_size;
    const int wi = valid ? stream_wakewords[sj] : -1;
    const bool live = wi >= 0 && wi < bank_W;   // an index outside the bank is an empty slot (the host checks it where it can see it)
    int lmax = 0;
    if (live)
        for (int j = 0; j < set_size; ++j) {
            const int wj = stream_wakewords[(size_t)s * set_size + j];
            if (wj >= 0 && wj < bank_W) lmax = max(lmax, bank_ww[wj].max_len);
        }
    RP_BANK_LIVE_LANE(lmax, 0)
}

// dtw_set_stream_kernel for a live-stream batch over MIXED sets (rp_stream_batch_new_mixed_sets; mfcc_size 16, what a model bank is): the
// stream also holds models, and its window is Lmax(s) frames with the COMBINED Lmax(s) over both rows, read from the per-stream table of
// stream_targets_kernel -- the wakeword bank alone cannot tell where a live window starts.  Everything else is dtw_set_stream_kernel's.
template <int K, int W>
__global__ __launch_bounds__(64) void dtw_mixed_stream_kernel(const BankWakeword *__restrict__ bank_ww, const int *__restrict__ bank_tlen,
                                                              const long long *__restrict__ bank_trow, const float *__restrict__ bank_unit,
                                                              const float *__restrict__ bank_raw, const float *__restrict__ mfcc,
                                                              const int32_t *__restrict__ stream_wakewords,
                                                              const BankWakeword *__restrict__ table, float *__restrict__ agg,
                                                              float *__restrict__ avg, uint32_t *__restrict__ fix, int bank_W, int set_size,
                                                              BankStreamScore q) {
    __shared__ float sl[kBankMaxTemplates * 64];   // a lane's scores (percentile modes), lane-minor
    __shared__ float Pb[13 * 64];                  // band of the reference-shaped cell
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x * 64u + lane, n_new = (uint32_t)q.n_new;
    const bool valid = row < (uint32_t)(q.S * (size_t)set_size * q.n_new);
    const uint32_t sj = valid ? row / n_new : 0u, i = row - sj * n_new;   // sj = s * set_size + j
    const uint32_t s = sj / (uint32_t)set_size;
    const int wi = valid ? stream_wakewords[sj] : -1;
    const bool live = wi >= 0 && wi < bank_W;   // an index outside the bank is an empty slot (the host checks it where it can see it)
    const int lmax = live ? table[s].max_len : 0;   // over both rows: at least this wakeword's window
    RP_BANK_LIVE_LANE(lmax, 1)
}

// table (with max_window, the longest window any stream of the batch may have: the combined history + 1): a batch over mixed sets, Lmax(s)
// from the table; nullptr: the set's own
template <int K, int W>
static hipError_t launch_set_stream_kw(hipStream_t st, const BankDev &b, const BankStreamScore &q, int set_size, const BankWakeword *table, unsigned blocks) {
    if constexpr (K == 16) {
        if (table) {
            hipLaunchKernelGGL((dtw_mixed_stream_kernel<K, W>), dim3(blocks), dim3(64), 0, st, b.ww, b.tlen, b.trow, b.unit, b.raw, q.mfcc, q.stream_wakeword,
                               table, q.agg, q.avg, q.fix, b.W, set_size, q);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((dtw_set_stream_kernel<K, W>), dim3(blocks), dim3(64), 0, st, b.ww, b.tlen, b.trow, b.unit, b.raw, q.mfcc, q.stream_wakeword,
                       q.agg, q.avg, q.fix, b.W, set_size, q);
    return hipGetLastError();
}

hipError_t launch_dtw_set_stream(hipStream_t st, const BankDev &b, const BankStreamScore &q, int set_size, const BankWakeword *table, int max_window) {
    if (q.S == 0 || q.n_new == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords) return hipErrorInvalidValue;
    if (b.W < 1 || (table && b.K != 16) || dtw_register_tile(b.K, q.band) <= 0) return hipErrorNotSupported;
    if (!table) max_window = b.max_len;   // the set's own Lmax(s): at most the bank's longest window
    else if (max_window < b.max_len) return hipErrorInvalidValue;
    // rows are 32-bit in the kernel; no window may start before its stream's row: Lmax(s) <= max_window
    if (q.S > 0x7fffffffULL / (q.n_new * (size_t)set_size) || q.first_new + 1 < (size_t)max_window || q.first_new + q.n_new > q.frame_pitch)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((q.S * (size_t)set_size * q.n_new + 63) / 64);
#define RP_SET(KK, WW) launch_set_stream_kw<KK, WW>(st, b, q, set_size, table, blocks)
#define RP_SET_BAND(KK) \
    switch (q.band) { case 3: return RP_SET(KK, 3); case 4: return RP_SET(KK, 4); case 5: return RP_SET(KK, 5); default: return RP_SET(KK, 6); }
    if (b.K == 5) { RP_SET_BAND(5) }
    if (b.K == 13) { RP_SET_BAND(13) }
    RP_SET_BAND(16)
#undef RP_SET_BAND
#undef RP_SET
}

}  // namespace rp
