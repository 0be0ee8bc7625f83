// rp_dtw_mixed.hip -- the reference side of a live-stream batch over MIXED sets (rp_stream_batch_new_mixed_sets): stream s holds wakeword
// references of a wakeword bank and models of a model bank on one detector, and its window is Lmax(s) frames, the longest over the live
// slots of BOTH rows.  dtw_set_stream_kernel (rp_dtw_set.hip) cannot serve: it takes Lmax(s) from the wakeword bank alone, and Lmax(s) decides
// where a live window starts.  The DTW walks are those of rp_dtw_bank.hip (rp_dtw_bank.h), operation for operation.
#include "rp_device.h"
#include "rp_dtw_bank.h"

namespace rp {

// dtw_set_stream_kernel's lane, operation for operation, at mfcc_size 16 (what a model bank is): lanes are consecutive rows of the flattened
// [S][set_size][n_new] space, windows minor; every lane walks the wakeword of its slot -- its own template walk, the per-lane gate,
// norm-range test, reference-shaped rescoring and percentile block.  The one difference: the window that ends at new frame i starts
// Lmax(s) - 1 frames before it with the COMBINED Lmax(s), read from the per-stream table of mixed_targets_kernel.  agg / avg
// [S][set_size][n_new]; an empty slot gets zero rows.
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
    const BankWakeword *bw = bank_ww + (live ? wi : 0);
    // the window ending at new frame i: Lmax(s) frames, the oldest first; this wakeword scores the oldest of them
    const float *xl = mfcc + (live ? ((size_t)s * q.frame_pitch + (q.first_new + i + 1 - (size_t)lmax)) * K : (size_t)0);
    const float own_athr = bw->avg_threshold;
    const float athr = own_athr == own_athr ? own_athr : q.avg_threshold;
    const int avg_e = bw->avg, T = live ? bw->count : 0, first = bw->first, ref_only = bw->ref_only, window_chk = bw->window_chk;
    const bool do_avg = live && avg_e >= 0 && athr != 0.f;   // wakeword_comp.rs:85
    const int mode = q.score_mode;

    float acc = 0.f, avg_sc = 0.f;
    bool scored = live;
    for (int ti = -1; __any(scored && ti < T); ++ti) {
        const bool act = scored && ti < T && (ti >= 0 || do_avg);
        float sc = 0.f, chk = 0.f;
        int L = 1;
        size_t off = 0;
        if (act) {
            const int e = ti < 0 ? avg_e : first + ti;
            L = bank_tlen[e];
            off = (size_t)bank_trow[e] * K;
            sc = bank_dtw<K, W, K>(xl, L, bank_unit + off, q.score_ref, chk);
            if (window_chk && chk > kDtwFixLimit) chk = bank_chk_window<K, K>(xl, L);
        }
        const bool slow = act && (ref_only || chk > kDtwFixLimit);
        const unsigned long long slow_mask = __ballot(slow);
        if (slow_mask) {   // wave-uniform
            if (slow) sc = bank_dtw_ref<K, W, K>(xl, L, bank_raw + off, q.score_ref, Pb, lane);
            if (lane == 0 && fix) atomicAdd(dtw_fix_stats(fix), (unsigned long long)__popcll(slow_mask));   // rp_ctx_dtw_ref_pairs
        }
        if (act) {
            if (ti < 0) {
                avg_sc = sc;
                // the averaged-template gate (wakeword_comp.rs:85-93), per lane
                if (q.gate && sc < athr) scored = false;
            } else if (mode == 1) acc = ti == 0 ? sc : fmaxf(acc, sc);   // Max
            else if (mode == 0) acc += sc;                               // Average: sequential sum in template order
            else sl[ti * 64 + lane] = sc;
        }
    }
    float a = 0.f;
    if (scored) {
        if (mode == 1) a = acc;
        else if (mode == 0) a = acc / (float)T;
        else {   // Median / percentiles: the lane sorts its column ascending, then the reference's f32 interpolation
            for (int j = 1; j < T; ++j) {
                const float x = sl[j * 64 + lane];
                int p = j - 1;
                while (p >= 0 && sl[p * 64 + lane] > x) { sl[(p + 1) * 64 + lane] = sl[p * 64 + lane]; --p; }
                sl[(p + 1) * 64 + lane] = x;
            }
            a = percentile_sorted(sl + lane, T, percentile_of_mode(mode), 64);
        }
    }
    // a window the gate rejected was never compared -> aggregate 0 (agg_store's rule, rp_dtw.hip); an empty slot: zero rows
    if (valid) {
        agg[row] = a;
        avg[row] = do_avg ? avg_sc : 0.f;
    }
}

template <int W>
static hipError_t launch_mixed_stream_w(hipStream_t st, const BankDev &b, const BankStreamScore &q, int set_size, const BankWakeword *table,
                                        unsigned blocks) {
    hipLaunchKernelGGL((dtw_mixed_stream_kernel<16, W>), dim3(blocks), dim3(64), 0, st, b.ww, b.tlen, b.trow, b.unit, b.raw, q.mfcc,
                       q.stream_wakeword, table, q.agg, q.avg, q.fix, b.W, set_size, q);
    return hipGetLastError();
}

hipError_t launch_dtw_mixed_stream(hipStream_t st, const BankDev &b, const BankStreamScore &q, int set_size, const BankWakeword *table,
                                   int max_window) {
    if (q.S == 0 || q.n_new == 0) return hipSuccess;
    if (set_size < 1 || set_size > kScanMaxWakewords || !table) return hipErrorInvalidValue;
    if (b.W < 1 || b.K != 16 || dtw_register_tile(b.K, q.band) <= 0) return hipErrorNotSupported;
    // rows are 32-bit in the kernel; no window may start before its stream's row: Lmax(s) <= max_window, the combined history + 1
    if (q.S > 0x7fffffffULL / (q.n_new * (size_t)set_size) || max_window < b.max_len || q.first_new + 1 < (size_t)max_window ||
        q.first_new + q.n_new > q.frame_pitch)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((q.S * (size_t)set_size * q.n_new + 63) / 64);
    switch (q.band) {
        case 3: return launch_mixed_stream_w<3>(st, b, q, set_size, table, blocks);
        case 4: return launch_mixed_stream_w<4>(st, b, q, set_size, table, blocks);
        case 5: return launch_mixed_stream_w<5>(st, b, q, set_size, table, blocks);
        default: return launch_mixed_stream_w<6>(st, b, q, set_size, table, blocks);
    }
}

}  // namespace rp
