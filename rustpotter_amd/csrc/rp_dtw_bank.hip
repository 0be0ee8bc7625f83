// rp_dtw_bank.hip -- dtw_bank_kernel: window scoring where stream s carries its OWN wakeword, bank[stream_wakeword[s]] -- the batched form of
// one `Rustpotter` per thread, each holding one personal wakeword (src/detector.rs:304-346; scoring as rp_dtw.hip: src/mfcc/dtw.rs:56-105 +
// comparator.rs + normalizer.rs + wakeword_comp.rs:22-27,77-139), and dtw_bank_stream_kernel: the same for the new windows of a live-stream
// batch, lanes = rows of many streams.  DESIGN.md §4.2c.
#include "rp_device.h"
#include "rp_dtw_bank.h"

namespace rp {

// One wave = one (stream, tile of 64 consecutive windows); lane = window.  The tile's 64 + max_len + W frames are staged in LDS once; the wave
// then walks its stream's wakeword: the averaged template first when it is to be scored, then the sample templates, folding the score_mode
// aggregate as it goes (running max / sum; the percentile modes keep the lane's scores in LDS, lane-minor).  The wakeword index is
// wave-uniform, so everything read through it -- the wakeword's record, template lengths, template rows -- is a scalar load.
// Written per stream row of win_pitch floats: agg (and avg) of the windows the stream has, zeros behind them and for streams without a wakeword.
// (The bank's arrays and the call's are separate __restrict__ parameters, not members of the structs: only then does the compiler know that
// the kernel's own stores cannot touch them and reads them with scalar loads.)
template <int K, int W>
__global__ __launch_bounds__(64) void dtw_bank_kernel(const BankWakeword *__restrict__ bank_ww, const int *__restrict__ bank_tlen,
                                                      const long long *__restrict__ bank_trow, const float *__restrict__ bank_unit,
                                                      const float *__restrict__ bank_raw, const float *__restrict__ mfcc,
                                                      const int32_t *__restrict__ stream_wakeword, float *__restrict__ agg, float *__restrict__ avg,
                                                      uint32_t *__restrict__ hot, uint32_t *__restrict__ fix, BankDev b, BankScore q, unsigned tiles) {
    constexpr int KP = (K % 2 == 0) ? K + 1 : K;  // odd pitch: conflict-free lane-strided LDS reads
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);               // [64 + b.max_len + 6][KP]
    float *sl = xs + (size_t)(64 + b.max_len + 6) * KP;        // [kBankMaxTemplates][64]: a lane's scores (percentile modes)
    float *Pb = sl + kBankMaxTemplates * 64;                   // [13][64]: band of the reference-shaped cell

    const unsigned tile = blockIdx.x % tiles;
    const size_t s = blockIdx.x / tiles;
    const int lane = threadIdx.x;
    const size_t wl = (size_t)tile * 64 + lane;
    float *agg_row = agg + s * q.win_pitch;
    float *avg_row = avg ? avg + s * q.win_pitch : nullptr;
    const int wi = stream_wakeword[s];
    const bool none = wi < 0 || wi >= b.W;   // an index outside the bank is "no wakeword" here (the host checks it where it can see it)
    const BankWakeword *bw = bank_ww + (none ? 0 : wi);
    const int max_len = none ? 0 : bw->max_len;
    const size_t n_win = (!none && q.n_frames >= (size_t)max_len) ? q.n_frames - (size_t)max_len + 1 : 0;
    if ((size_t)tile * 64 >= n_win) {
        if (wl < q.win_pitch) {
            agg_row[wl] = 0.f;
            if (avg_row) avg_row[wl] = 0.f;
        }
        return;
    }
    {
        const int n_stage = 64 + max_len + W;
        const float *src = mfcc + s * q.n_frames * K;
        const size_t w0 = (size_t)tile * 64;
        for (int i = lane; i < n_stage * K; i += 64) {
            const int f = i / K, k = i - f * K;
            const size_t g = w0 + f;
            xs[f * KP + k] = g < q.n_frames ? src[g * K + k] : 0.f;
        }
    }
    __syncthreads();
    const float *xl = xs + lane * KP;
    const bool valid = wl < n_win;
    const float own_thr = bw->threshold, own_athr = bw->avg_threshold;
    const float thr = own_thr == own_thr ? own_thr : q.threshold;
    const float athr = own_athr == own_athr ? own_athr : q.avg_threshold;
    const int avg_e = bw->avg, T = bw->count, first = bw->first, ref_only = bw->ref_only, window_chk = bw->window_chk;
    const bool do_avg = avg_e >= 0 && (q.avg_mode == 1 || (q.avg_mode == 2 && athr != 0.f));   // wakeword_comp.rs:85
    const int mode = q.score_mode;

    float acc = 0.f, avg_sc = 0.f;
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
            // the averaged-template gate (wakeword_comp.rs:85-93) at wave granularity, as dtw_generic_kernel: when none of the wave's windows
            // passed, the sample templates are not compared at all
            if (q.gate && !__any(valid && !(sc < athr))) { scored = false; break; }
        } else if (mode == 1) acc = ti == 0 ? sc : fmaxf(acc, sc);   // Max
        else if (mode == 0) acc += sc;                               // Average: sequential sum in template order
        else sl[ti * 64 + lane] = sc;
    }
    float a = 0.f;
    if (scored) {
        if (mode == 1) a = acc;
        else if (mode == 0) a = acc / (float)T;
        else {   // Median / percentiles: the lane sorts its column ascending, then the reference's f32 interpolation
            for (int i = 1; i < T; ++i) {
                const float x = sl[i * 64 + lane];
                int j = i - 1;
                while (j >= 0 && sl[j * 64 + lane] > x) { sl[(j + 1) * 64 + lane] = sl[j * 64 + lane]; --j; }
                sl[(j + 1) * 64 + lane] = x;
            }
            a = percentile_sorted(sl + lane, T, percentile_of_mode(mode), 64);
        }
    }
    // agg_store's rules (rp_dtw.hip): a window the gate rejected was never compared -> aggregate 0; a window that can fire raises the stream's flag
    const bool gated = q.gate && do_avg && avg_sc < athr;
    if (gated) a = 0.f;
    if (wl < q.win_pitch) {
        agg_row[wl] = valid ? a : 0.f;
        if (avg_row) avg_row[wl] = (valid && do_avg) ? avg_sc : 0.f;
    }
    if (hot && __any(valid && !gated && a > thr) && lane == 0) hot[s] = 1u;
}

template <int K, int W>
static hipError_t launch_bank_kw(hipStream_t st, const BankDev &b, const BankScore &q, unsigned blocks, unsigned tiles, size_t lds) {
    const auto kernel = dtw_bank_kernel<K, W>;
    if (lds > 64 * 1024)
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), 160 * 1024); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, st, b.ww, b.tlen, b.trow, b.unit, b.raw, q.mfcc, q.stream_wakeword, q.agg, q.avg, q.hot, q.fix, b, q, tiles);
    return hipGetLastError();
}

hipError_t launch_dtw_bank(hipStream_t st, const BankDev &b, const BankScore &q) {
    if (q.S == 0 || q.win_pitch == 0) return hipSuccess;
    if (dtw_register_tile(b.K, q.band) <= 0) return hipErrorNotSupported;
    const size_t tiles = (q.win_pitch + 63) / 64, blocks = tiles * q.S;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = dtw_bank_lds_bytes(b.K, b.max_len);
    if (lds > 160 * 1024) return hipErrorMemoryAllocation;
#define RP_BANK(KK, WW) launch_bank_kw<KK, WW>(st, b, q, (unsigned)blocks, (unsigned)tiles, lds)
#define RP_BANK_BAND(KK) \
    switch (q.band) { case 3: return RP_BANK(KK, 3); case 4: return RP_BANK(KK, 4); case 5: return RP_BANK(KK, 5); default: return RP_BANK(KK, 6); }
    if (b.K == 5) { RP_BANK_BAND(5) }
    if (b.K == 13) { RP_BANK_BAND(13) }
    RP_BANK_BAND(16)
#undef RP_BANK_BAND
#undef RP_BANK
}

// dtw_bank_kernel for a live-stream batch (rp_stream_batch_new_bank).  A stream brings only 3 * n_chunks new windows per call, so a wave per
// (stream, 64 windows) would leave most lanes idle; here, as in the GX forms of rp_dtw.hip, the wave's 64 lanes are consecutive rows of the
// flattened [S][n_new] space: a wave straddles streams and therefore wakewords.  Every lane reads its stream's index and wakeword record,
// points at its window in the batch's MFCC rows in global memory (frame_pitch frames a stream) and walks ITS wakeword -- the averaged
// template first when it is to be scored, then the sample templates -- so template count, template length and template rows are per-lane
// values: the template loop runs to the wave's largest count, bank_dtw's row loop to the wave's longest template, both under the lane mask,
// and template rows come by vector loads.  The cell arithmetic is bank_dtw's, operation for operation: a stream gets the bits dtw_bank_kernel
// gives it.  Norm-range test, reference-shaped rescoring (the lanes that need it only) and the percentile block as there; the gate is per lane.
template <int K, int W>
__global__ __launch_bounds__(64) void dtw_bank_stream_kernel(const BankWakeword *__restrict__ bank_ww, const int *__restrict__ bank_tlen,
                                                             const long long *__restrict__ bank_trow, const float *__restrict__ bank_unit,
                                                             const float *__restrict__ bank_raw, const float *__restrict__ mfcc,
                                                             const int32_t *__restrict__ stream_wakeword, float *__restrict__ agg,
                                                             float *__restrict__ avg, uint32_t *__restrict__ fix, int bank_W, BankStreamScore q) {
    __shared__ float sl[kBankMaxTemplates * 64];   // a lane's scores (percentile modes), lane-minor
    __shared__ float Pb[13 * 64];                  // band of the reference-shaped cell
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x * 64u + lane, n_new = (uint32_t)q.n_new;
    const bool valid = row < (uint32_t)(q.S * q.n_new);
    const uint32_t s = valid ? row / n_new : 0u, i = row - s * n_new;
    const int wi = valid ? stream_wakeword[s] : -1;
    const bool live = wi >= 0 && wi < bank_W;   // an index outside the bank is "no wakeword" (the host checks it where it can see it)
    RP_BANK_LIVE_LANE(bw->max_len, 0)
}

template <int K, int W>
static hipError_t launch_bank_stream_kw(hipStream_t st, const BankDev &b, const BankStreamScore &q, unsigned blocks) {
    hipLaunchKernelGGL((dtw_bank_stream_kernel<K, W>), dim3(blocks), dim3(64), 0, st, b.ww, b.tlen, b.trow, b.unit, b.raw, q.mfcc, q.stream_wakeword,
                       q.agg, q.avg, q.fix, b.W, q);
    return hipGetLastError();
}

hipError_t launch_dtw_bank_stream(hipStream_t st, const BankDev &b, const BankStreamScore &q) {
    if (q.S == 0 || q.n_new == 0) return hipSuccess;
    if (b.W < 1 || dtw_register_tile(b.K, q.band) <= 0) return hipErrorNotSupported;
    // rows are 32-bit in the kernel; no window may start before its stream's row
    if (q.S > 0x7fffffffULL / q.n_new || q.first_new + 1 < (size_t)b.max_len || q.first_new + q.n_new > q.frame_pitch) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((q.S * q.n_new + 63) / 64);
#define RP_BANK(KK, WW) launch_bank_stream_kw<KK, WW>(st, b, q, blocks)
#define RP_BANK_BAND(KK) \
    switch (q.band) { case 3: return RP_BANK(KK, 3); case 4: return RP_BANK(KK, 4); case 5: return RP_BANK(KK, 5); default: return RP_BANK(KK, 6); }
    if (b.K == 5) { RP_BANK_BAND(5) }
    if (b.K == 13) { RP_BANK_BAND(13) }
    RP_BANK_BAND(16)
#undef RP_BANK_BAND
#undef RP_BANK
}

}  // namespace rp
