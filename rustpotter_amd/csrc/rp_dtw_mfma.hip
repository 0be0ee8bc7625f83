// rp_dtw_mfma.hip -- dtw_mfma_kernel: the banded DTW of mfcc_size 5 with the cosine costs on the matrix cores (DESIGN.md §4.2,
// round 3).  Same scoring as dtw_band_kernel (src/mfcc/dtw.rs:56-105 + comparator.rs:15-48 + normalizer.rs:17-29 +
// wakeword_comp.rs:22-37), other arithmetic for the cell cost:
//
//   * dtw_band_kernel spends 5 of the 8 issue slots of a band cell of a template pair on v_pk_fma_f32 for `1 - a.x` -- at the f32
//     FMA peak of the vector pipe (tools/scratch/valu_rate_probe.hip: 4.7 cycles per packed op, 4.2 per v_min3_f32).  Here the costs of
//     a whole band COLUMN come out of v_mfma_f32_32x32x16_f16 and the vector pipe only runs the recurrence.
//   * A wave owns 32 windows x one chunk of up to 8 same-length templates.  Lane l = (window l & 31, half h = l >> 5) runs the
//     recurrence of templates 4h..4h+3 (two packed pairs) of its window: the MFMA's C/D layout (col = lane & 31,
//     row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) puts exactly those costs into that lane, pairs in consecutive registers.
//   * Column-major sweep: step c takes window frame c against the 2W template rows of its band (rows c-W+1 .. c+W).  M = 8
//     templates x 12 circular row slots (row r lives in slot r mod 12) = 3 tiles of 32 rows, N = 32 windows, K = 16 f16 slots
//     = one instruction per tile.  A (the negated unit rows, split on the host, 256 B per template row in LDS) changes by one
//     row per template and column: one tile's operand is re-read per column.
//   * Precision: x = x0 + x1, a = a0 + a1 with x0 = rtz_f16(x), x1 = rtz_f16(x - x0) (22 significant bits; round 4: the template side rounds
//     both parts to nearest and carries the gain that undoes the window side's truncation, rp_device.h pk_f16_second); the slots hold
//     x0 a0, x1 a0, x0 a1 for the five components (15) and 1.0 x 1.0, accumulated in f32 on C = 0: the instruction leaves
//     1 - a.x with an error below 2^-20 (measured against the f32 CPU restatement: scores within 1e-6; the parity gate is 1e-5).
//     Lane (n, h) centres, scales and splits only components (0, 1) or (3, 4) and component 2; the two partial squared norms
//     meet through v_permlane32_swap.  (The three-part form builds a WHOLE frame per lane every two columns instead: RP_W_*, below.)
//   * Software pipeline per column c: the A tile of column c+1 is re-read, the cells of column c run (two independent chains of
//     v_min3_f32 x2 + add x2 per cell), each tile's MFMA for column c+1 is issued right after the last cell that reads the tile, and
//     the frame of column c+2 is prepared in ten pieces between the cells (three-part form: the frames of a column PAIR, nine pieces over two columns).  Columns are unrolled 12 at a time so that every
//     slot, tile and band index is a compile-time register.
//   * Two arithmetics (P3, round 6; chosen by the context, rp_ctx_set_arithmetic).  P3 = true, the default (RP_ARITH_F32_MATRIX): f32-GRADE products.
//     Both operands are split into THREE bf16 parts, exactly (x0 = x & 0xffff0000, r = x - x0, x1 = r & 0xffff0000, x2 = r - x1: 3 x 8 significant
//     bits = an f32's 24; the template rows on the host, rounded to nearest), and the six partial products x_i a_j with i + j <= 2 of the five
//     components + 1.0 x 1.0 fill 31 of the 32 k-slots of TWO v_mfma_f32_32x32x16_bf16 chained on one accumulator (the second one band cell
//     after the first).  What is dropped (x1 a2 + x2 a1 + x2 a2) is below 2^-22 of a product, 2^-25.7 rms -- an f32 multiply rounds by up to
//     2^-24; tests/test_gpu_dtw_f64.py holds the scores to the strict-f32 oracle's own distance from an f64 evaluation.  The window side's two
//     operands are one run of six registers (the middle two shared), the A image is 512 bytes per template row (append_mfma_image3,
//     rp_ctx.cpp); twelve waves per workgroup = three per SIMD at 168 registers with nothing spilled where twelve waves' frame stages fit beside
//     the A image, eight (184 registers) where they do not, in a live-stream call, or under RP_MFMA3_WAVES=8 (see the launcher; THREE WAVES below).  P3 = false (RP_ARITH_FAST_SPLIT, opt-in): the two-part f16 form
//     described above, 22-bit products.
//   * Two shapes (NT): eight template slots as described (chunks of 5..8 templates, band 3..5), or four (chunks of 3..4, band 5): a
//     tile is then 8 row slots x 4 templates, 16 circular row slots = 2 tiles, one template pair per lane, columns unrolled 16 at a time, twelve
//     waves per workgroup (eight where twelve waves' frame stages no longer fit beside the A image) in both arithmetics.  mfcc_size 13 / 16 have their own K axis: rp_dtw_mfma_wide3.hip / rp_dtw_mfma_wide.hip.
//   * THREE WAVES (168 registers): the third wave per SIMD hides the cell-to-cell dependence of the recurrence, and a column's state -- band
//     costs 40, accumulators 48, A operands 24, window operands 12 -- is 124 registers before anything else.  What makes the rest fit: (1) nothing
//     that is only a function of the lane or of a kernel argument is HELD -- lane constants come from fresh_lane_id() once per tile and per part of
//     the column sweep, the output row is worked out again behind the columns, float forms and reciprocals of uniform values are made where they are
//     used (not_hoisted) -- the compiler otherwise computes them once per kernel and spills them; (2) the early abandon of detect-only calls is a
//     kernel of its own for these builds (mfma_abandon_apart, dtw_mfma_abandon_kernel): its state is ten values across the column loop; (3) the
//     staged eight-slot build holds the second k-step's A operand only for the tile that takes the column's new row and reads the two others'
//     from LDS a cell before their matrix instructions (mfma_late_a2: +2 ds_read_b128 per column, -8 registers); (4) a frame's split runs in two
//     pieces instead of four, so that x0_ and y_ never cross a band cell.  No floating-point operation moved: bits as before.
//   * BUILD: the 12 / 16-column blocks are `#pragma unroll` loops whose bodies exceed the compiler's budget for pragma-requested full
//     unrolling; this file is compiled with -mllvm -pragma-unroll-threshold=200000 (Makefile FILE_FLAGS_rp_dtw_mfma.hip).  Without it the
//     three-part four-slot build keeps a rolled loop, indexes its accumulators at run time and spills 13 709 values.
// Measured (tools/scratch/dtw_mfma_probe2.hip, 8 192 streams x 288 windows x 8 templates of 100 frames): 1.62 ms against 2.36 ms at
// dtw_band_kernel's C3 rate; VALU-issue bound (SQ_ACTIVE_INST_VALU = 100 % of the SIMD cycles), matrix pipe 21 % busy.  In the product
// at C3: 19.5 ms (vector kernels) -> 11.6-11.9 (two-part form) / 14.4-15.3 (three-part form, matrix pipe 39 % busy) (DESIGN.md §4.2,
// profiles/r06_final_*).
#include "rp_device.h"

#include <cstdlib>

namespace rp {

namespace {

typedef unsigned u32x6 __attribute__((ext_vector_type(6)));   // the window side's run of six registers (P3)

// The lane's index in its wave from nothing that lives in a register: two v_mbcnt on a mask the compiler takes for unknown, so that two calls
// are two values and neither is kept from one to the other (threadIdx.x & 63 is ONE value, alive from the kernel's entry to its last use).
__device__ __forceinline__ int fresh_lane_id() {
    unsigned ones = ~0u;
    asm volatile("" : "+s"(ones));
    return (int)__builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
}
// a wave-uniform value as the compiler must take it where it stands: what is computed from it (a float form, a reciprocal: vector registers)
// is computed there and not once per kernel
template <class T> __device__ __forceinline__ T not_hoisted(T v) {
    asm volatile("" : "+s"(v));
    return v;
}
// a 64-bit value every lane holds alike, moved to scalar registers
__device__ __forceinline__ size_t wave_uniform(size_t v) {
    return ((size_t)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32)) << 32) | (size_t)__builtin_amdgcn_readfirstlane((unsigned)v);
}

constexpr int kMK = 5;         // MFCC coefficients per frame
constexpr int kMWin = 32;      // windows per wave
// NT template slots per chunk: 8 (chunks of 5..8 templates; a tile of 32 rows = 4 row slots x 8 templates, 12 circular row slots = 3
// tiles, a lane runs two template pairs) or 4 (chunks of 3..4; a tile = 8 row slots x 4 templates, 16 row slots = 2 tiles, one pair)
constexpr int mfma_slots(int nt) { return nt == 8 ? 12 : 16; }
constexpr int mfma_tiles(int nt) { return nt == 8 ? 3 : 2; }
constexpr int kMSlotsMax = 16;  // rows of zero padding behind a chunk's A image
// accumulator register of (row slot, template pair p, pair element e) in its tile: the C/D layout puts row (reg & 3) + 8 (reg >> 2) +
// 4 (lane >> 5) into `reg` of lane half lane >> 5.  NT = 8: row = 8 (slot % 4) + 4 h + (2 p + e); NT = 4: row = 8 (s >> 1) + 4 h +
// 2 (s & 1) + e with s = slot % 8.
constexpr int mfma_acc_reg(int nt, int slot, int p, int e) {
    return nt == 8 ? 4 * (slot % 4) + 2 * p + e : 4 * ((slot % 8) >> 1) + 2 * (slot & 1) + e;
}

#ifdef RP_MFMA_CVT_BACK  // A/B build only: x0 as f32 by converting the f16 back (see RP_X0F)
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float lo_f32(unsigned p) { return (float)__builtin_bit_cast(fp16x2, p)[0]; }
__device__ __forceinline__ float hi_f32(unsigned p) { return (float)__builtin_bit_cast(fp16x2, p)[1]; }
#endif

// last band position q of column phase u whose MFMA row slot (u + q + NS - W + 2) mod NS lies in tile g; -1: the tile is not read
template <int W, int NT>
__host__ __device__ constexpr int mfma_last_use(int u, int g) {
    int last = -1;
    for (int q = 0; q < 2 * W; ++q)
        if (((u + q + mfma_slots(NT) - W + 2) % mfma_slots(NT)) / (32 / NT) == g) last = q;
    return last;
}

// Which instantiations build the window operand one whole frame per lane and column pair (RP_W_*, in the kernel): the builds of the three-part
// form but one -- the twelve-wave eight-slot build that reads its frames from global memory (RP_MFMA3_WAVES=12 in a live-stream call), where
// the pair ring of ten registers does not fit 168 registers (59 spilled values without it): that one keeps the per-column build (RP_P*), as does
// the two-part form, whose split is two conversions per component pair and not what this saves on.
constexpr bool mfma_whole_frame(int nw, bool gx, int nt, bool p3) { return p3 && !(gx && nw == 12 && nt == 8); }
// Which instantiations read the second k-step's A operand of a tile from LDS right before its matrix instruction instead of holding it: the staged
// twelve-wave eight-slot builds of the three-part form.  Only the tile that takes a column's new row is re-read at the head of the column (RP_AREF);
// the two others hold rows that sit where they sat, at an offset that is the same for every lane but for jj rows: one address register + an
// immediate, two more 16-byte reads per column, and eight registers of operand held no longer.
constexpr bool mfma_late_a2(int nw, bool gx, int nt, bool p3) { return p3 && nw == 12 && nt == 8 && !gx; }
// the band cell of column phase u after which tile g's second-step operand is requested: one cell before the tile's first matrix instruction
template <int W, int NT>
__host__ __device__ constexpr int mfma_a2_request(int u, int g) {
    const int lu = mfma_last_use<W, NT>(u, g);
    return lu < 0 ? 2 * W - 2 : (lu < 1 ? 0 : lu - 1);
}
// rows between the newest row (slot sn) and the one row slot 0 + jj of tile g holds, plus jj (g is not sn's tile: no lane wraps differently)
constexpr int mfma_a2_back(int sn, int g, int nt) { return sn - (32 / nt) * g < 0 ? sn - (32 / nt) * g + mfma_slots(nt) : sn - (32 / nt) * g; }

// Which instantiations leave the early abandon of detect-only calls to a kernel of its own (dtw_mfma_abandon_kernel): the twelve-wave builds of
// the whole-frame form.  At 168 registers the abandon state -- which of a lane's templates are real, which the averaged one, the cost bound, the
// wave's verdict -- is ten values held across the column loop, and a call whose result is its score arrays (abandon_nc = +inf) never reads them.
constexpr bool mfma_abandon_apart(int nw, bool gx, int nt, bool p3) { return nw == 12 && mfma_whole_frame(nw, gx, nt, p3); }

}  // namespace

// One workgroup = NW waves on one chunk (its A image is staged once); waves take the 32-entry tiles of the flattened
// (stream, window) space from an atomic counter.  GX = false: a tile's frames are staged in LDS, a tile may straddle two streams
// (n_win >= 32).  GX = true: lanes read their window's frames from global memory (live-stream batches: a few windows per
// stream; LIST mode of the averaged-template gate: list[] holds the rows that passed, *count of them).  list == nullptr with a
// count: DENSE mode of the gate -- the launch does nothing unless *count >= dense_min; LIST mode does nothing when the list is
// dense (GateList, rp_kernels.h).  abandon_nc < inf: early abandon of detect-only calls -- every 12 (16) columns a wave stops when the
// cheapest band cell of every (window, template) it holds is past abandon_nc * (m + n), writing score 0 (cell costs are >= 0 and
// every warping path crosses every column, so that cell bounds the final cost from below; the averaged template never stops).
// static_rounds: tiles a wave takes by its own index before it turns to the counter (mfma_static_rounds, rp_kernels.h).  agg_out != null:
// the chunk holds every sample template of the reference -- the kernel also writes ScoreMode::Max of a window's scores and raises the
// stream's hot flag (DtwFusedAgg, rp_kernels.h).
// RP_MFMA_TRACE (variant builds only, tools/r4_mfma_timeline.py): wave 0 and the last wave of every workgroup stamp the constant
// 100 MHz clock at the kernel's phase boundaries into the tail of the counter block (DtwWork::sched words 1024..4095, the first 96 workgroups: the
// list words of DtwWork::fix start right behind): where a short
// launch spends its fixed cost.  Never defined in the product.
#ifdef RP_MFMA_TRACE
#define RP_TRACE(slot)                                                                                                        \
    do {                                                                                                                      \
        if ((threadIdx.x & 63) == 0 && ((threadIdx.x >> 6) == 0 || (threadIdx.x >> 6) == NW - 1) && blockIdx.x < 96)   /* 96 x 2 x 8 stamps end with the counter block */          \
            reinterpret_cast<unsigned long long *>(sched + 1024)[(blockIdx.x * 2 + ((threadIdx.x >> 6) ? 1 : 0)) * 8 + (slot)] = \
                __builtin_amdgcn_s_memrealtime();                                                                             \
    } while (0)
#else
#define RP_TRACE(slot)
#endif

#ifndef RP_MFMA_WAVES_PER_EU   // experiment builds: cap every instantiation at the registers of N waves per SIMD (3: 168), e.g. to leave room
#define RP_MFMA_WAVES_PER_EU 0 // for another kernel's waves beside an eight-wave workgroup
#endif
#if RP_MFMA_WAVES_PER_EU
#define RP_MFMA_OCC __attribute__((amdgpu_waves_per_eu(RP_MFMA_WAVES_PER_EU, RP_MFMA_WAVES_PER_EU)))
#else
#define RP_MFMA_OCC
#endif
// the kernel's parameters, once for the body and the two kernels around it
#define RP_MFMA_PARAMS                                                                                                                       \
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_frames_total, size_t total_tiles, unsigned n_chunks, int chunk_base,        \
    size_t first_win, size_t n_win, size_t out_win_pitch, const DtwChunk *__restrict__ chunks, const uint4 *__restrict__ aimg, int T,        \
    float score_ref, float *__restrict__ scores, float *__restrict__ avg, size_t n_streams, int max_len, const uint32_t *__restrict__ list, \
    const uint32_t *__restrict__ count, uint32_t dense_min, float abandon_nc, uint32_t *__restrict__ sched, unsigned static_rounds,         \
    float *__restrict__ agg_out, uint32_t *__restrict__ agg_hot, float agg_threshold, uint32_t *__restrict__ fix
#define RP_MFMA_ARGS                                                                                                                         \
    mfcc, frame_pitch, n_frames_total, total_tiles, n_chunks, chunk_base, first_win, n_win, out_win_pitch, chunks, aimg, T, score_ref,      \
    scores, avg, n_streams, max_len, list, count, dense_min, abandon_nc, sched, static_rounds, agg_out, agg_hot, agg_threshold, fix
// AB: early abandon compiled in (abandon_nc < inf then switches it on); false: the call's score arrays are its result, nothing stops early
template <int W, int NW, bool GX, int NT, bool P3, bool AB>
__device__ __forceinline__ void dtw_mfma_body(RP_MFMA_PARAMS) {
    constexpr int K = kMK, B = 2 * W, NS = mfma_slots(NT), NTILE = mfma_tiles(NT), SPT = 32 / NT, NP = NT / 4;
    constexpr int kRowBytes = P3 ? kDtwMfma3RowBytes : kDtwMfmaRowBytes;
#ifndef RP_MFMA_GX_PD  // A/B builds: 1 = the one-column look-ahead of the staged form
    constexpr int PD = GX ? (NS % 3 == 0 ? 3 : 4) : 1;  // columns a frame is requested ahead of its use (RP_P0)
#else
    constexpr int PD = GX ? RP_MFMA_GX_PD : 1;
#endif
    static_assert(NS % PD == 0, "the frame ring's slot must be a compile-time index");
    // WF: the window operand is built one WHOLE frame per lane and column pair (RP_W_*, below); false: every lane builds its half of every column (RP_P*)
    constexpr bool WF = mfma_whole_frame(NW, GX, NT, P3);
    constexpr int PP = GX ? 2 : 1;  // WF: pairs a frame pair is requested ahead of its use
    constexpr bool A2L = mfma_late_a2(NW, GX, NT, P3);
    static_assert(NS % (2 * PP) == 0, "the pair ring's slot must be a compile-time index");
    static_assert(NT == 8 || NT == 4, "template slots per chunk");
    static_assert(B + 2 <= NS, "the band and its two neighbours must fit the circular row slots");
    size_t total_entries = n_streams * n_win;
    if (list) {
        const uint32_t n_listed = *count;
        if (dense_min && n_listed >= dense_min) return;
        total_entries = n_listed;
        total_tiles = ((size_t)n_listed + kMWin - 1) / kMWin;
    } else if (count && *count < dense_min) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    RP_TRACE(0);
    const unsigned ci = blockIdx.x % n_chunks;
    const unsigned n_groups = gridDim.x / n_chunks;
    const DtwChunk *ch = chunks + chunk_base + ci;
    const int L = ch->len;  // m == n == L
    const int a_bytes = (max_len + kMSlotsMax) * kRowBytes;
    const int xs_floats = dtw_mfma_stage_floats(max_len);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    dtw_load_aimg<64 * NW>(smem, aimg, P3 ? ch->aimg3_off : ch->aimg_off, (L + kMSlotsMax) * kRowBytes / 16, tid);
    __syncthreads();
    RP_TRACE(1);
    float *xs = reinterpret_cast<float *>(smem + a_bytes) + wave * xs_floats;
    (void)xs;
    // The early abandon's state, once per kernel (AB only): the template ids are loads from global memory, and a round trip to it in every tile is
    // 2.5 % of a live-stream call of eight chunks
    const int hAb = fresh_lane_id() >> 5;
    const float abandon_cost = abandon_nc * (float)(L + L);
    // which of this lane's templates (NT / 2 of them) can keep a wave alive: real ones; the averaged template (tid >= T) always does
    bool slot_real[2 * NP], slot_avg[2 * NP];
#pragma unroll
    for (int e = 0; e < 2 * NP; ++e) {
        slot_real[e] = 2 * NP * hAb + e < ch->count;
        slot_avg[e] = slot_real[e] && ch->tid[2 * NP * hAb + e] >= T;
    }

    uint32_t *next_tile = sched + 2 * (chunk_base + ci);
    unsigned round = 0;
    const size_t chunk_waves = (size_t)n_groups * NW;  // waves working on this chunk
    for (;;) {
        const size_t tile = wave_uniform(dtw_next_tile<NW>(next_tile, round, static_rounds, chunk_waves, n_chunks, wave, fresh_lane_id()));
        if (tile >= not_hoisted(total_tiles)) break;  // a 64-bit >= is a vector compare: no copy of the bound in vector registers across tiles
        // The lane's constants are derived per tile, and per phase of a tile, from lane ids the compiler cannot trace back: computed once per
        // kernel they are a dozen registers held (at three waves per SIMD: spilled) across every tile for the sake of a dozen instructions
        const int lane_ = fresh_lane_id();
        const int n = lane_ & 31, h = lane_ >> 5;
        // ---- lanes -> (stream, window): here for the frames and, in LDS-staged tiles, once more behind the columns for the output row -- the
        // stream, the window and the validity of a lane are four registers that nothing in between reads, and a few scalar operations to make
        // again.  From global memory (GX) they are a list lookup and a 64-bit division per lane (2 % of a live-stream call when made twice): kept.
        const size_t f0 = tile * kMWin;
        const size_t n_win_ = not_hoisted(n_win);  // the division's reciprocal is per tile, not three vector registers per kernel
        // LDS-staged tiles: the tile's first (stream, window) and its up to two stream segments, wave-uniform
        const size_t sA = GX ? 0 : f0 / n_win_;
        const int wA = GX ? 0 : (int)(f0 - sA * n_win_);
        const int nA = (int)n_win_ - wA < kMWin ? (int)n_win_ - wA : kMWin;
        const int nB = (nA < kMWin && sA + 1 < n_streams) ? kMWin - nA : 0;
        const int segA = nA + L + 3;
        auto locate = [&](int n_, size_t &s_, int &w_) -> bool {
            if (GX) {
                size_t f = f0 + n_;
                const bool valid_ = f < total_entries;
                if (list) f = list[valid_ ? f : total_entries - 1];  // row ids s * n_win_ + w of the windows that passed the gate
                s_ = valid_ ? f / n_win_ : 0;
                w_ = valid_ ? (int)(f - s_ * n_win_) : 0;
                return valid_;
            }
            const bool inA = n_ < nA;
            s_ = inA ? sA : sA + 1;
            w_ = inA ? wA + n_ : n_ - nA;
            return inA || (n_ - nA < nB);
        };
        const float *xw;
        size_t s_gx;
        int w_gx;
        const bool valid = locate(n, s_gx, w_gx);
        if (GX) xw = mfcc + (s_gx * frame_pitch + first_win + (size_t)w_gx) * K;  // columns up to L + 8 are read ahead: the caller's frame array ends with 64 frames of slack
        if (!GX) {
            // stage the frames of up to two stream segments (columns L + 1 .. L + 3 are read ahead, never used)
            // four loads in flight per wait: left one by one, a tile's ~11 loads per lane were as many L2 round trips -- nothing covers
            // them in the first round of a short launch, where every wave of the chip stages at the same time
            auto stage =[&](const float *src, size_t g0, int n_floats, float *dst) {
                for (int i0 = lane_; i0 < n_floats; i0 += 256) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = i0 + 64 * j;
                        v[j] = (i < n_floats && g0 + (size_t)(i / K) < n_frames_total) ? src[g0 * K + i] : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (i0 + 64 * j < n_floats) dst[i0 + 64 * j] = v[j];
                }
            };
            stage(mfcc + sA * frame_pitch * K, first_win + wA, segA * K, xs);
            if (nB > 0) stage(mfcc + (sA + 1) * frame_pitch * K, first_win, (nB + L + 3) * K, xs + segA * K);
            wave_lds_sync();
            xw = xs + (n < nA ? n : (valid ? segA + n - nA : 0)) * K;
        }
        const float *xa = xw + (h ? 3 : 0);  // this half's two components; component 2 at xw + 2
        const float *x2 = xw + 2;
        // MfccNormalizer::normalize, src/mfcc/normalizer.rs:17-29: sequential column sums (of this lane's three components)
        float mua = 0.f, mub = 0.f, mu2 = 0.f;
#ifndef RP_MFMA_GX_MEAN_UNROLL
#define RP_MFMA_GX_MEAN_UNROLL 20
#endif
#ifndef RP_MFMA_MEAN_UNROLL
#define RP_MFMA_MEAN_UNROLL 8
#endif
        constexpr int kMeanUnroll = GX ? RP_MFMA_GX_MEAN_UNROLL : RP_MFMA_MEAN_UNROLL;  // from global memory: 20 frames in flight per wait (an L2 round trip each), sums in the same order
#pragma unroll kMeanUnroll
        for (int i = 0; i < L; ++i) { mua += xa[i * K]; mub += xa[i * K + 1]; mu2 += x2[i * K]; }
        const float fL = (float)not_hoisted(L);
        mua = mua / fL; mub = mub / fL; mu2 = mu2 / fL;
        // WF: the lane centres all five components; the two means it did not sum come from the other half (same sums, same order, same bits)
        float mu_[K] = {0.f, 0.f, 0.f, 0.f, 0.f};
        (void)mu_;
        if (WF) {
            const auto sa_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(mua), __float_as_uint(mua), false, false);
            const auto sb_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(mub), __float_as_uint(mub), false, false);
            mu_[0] = __uint_as_float(sa_[0]); mu_[3] = __uint_as_float(sa_[1]);
            mu_[1] = __uint_as_float(sb_[0]); mu_[4] = __uint_as_float(sb_[1]);
            mu_[2] = mu2;
        }
        const float *xh = xw + h * K;  // WF: half h holds the second column of a pair
        (void)xh;
        // The lane's constants of the columns, from a lane id of their own -- those of the staging above are dead by here -- and once more for
        // each part of the column sweep (the guarded first block, the blocks of the loop, the tail): what one part has derived from them,
        // addresses mostly, is not held through the next.
        // A operand: this lane supplies row m = lane & 31 of a tile, k half = lane >> 5.  NT = 8: m = 8 jj + 4 h' + r' = (row slot jj of the
        // tile, template 4 h' + r'); NT = 4: m = 8 G + 4 h' + 2 sp + e = (row slot 2 G + sp, template 2 h' + e).
        // dl[e]: byte offset back to the row this lane's slot holds when the newest row sits in slot e of its tile.
        // P3 without whole frames: register 3 of the first operand holds (x0, x1) of component 2 in half 0 and (x2, x0) in half 1 -- one v_perm
        // of (t, x0) with a per-half selector, t = r1 - (r1 & mask_c2): r1 itself in half 0 (its upper 16 bits ARE x1), x2 in half 1
#define RP_LANE_CONSTS()                                                                                                      \
        const int laneA_ = fresh_lane_id();                                                                                   \
        const int hA = laneA_ >> 5;                                                                                           \
        const bool upper = hA != 0;                                                                                           \
        const int mrow = laneA_ & 31;                                                                                         \
        const int jj = NT == 8 ? mrow >> 3 : 2 * (mrow >> 3) + ((mrow >> 1) & 1);                                             \
        const int tA = NT == 8 ? ((mrow >> 2) & 1) * 4 + (mrow & 3) : ((mrow >> 2) & 1) * 2 + (mrow & 1);                     \
        const unsigned a_lane = (unsigned)(hA * 128 + tA * 16);                                                               \
        const unsigned a2_lane = a_lane + 256u + (unsigned)jj * kRowBytes;  /* A2L: second-step operand of the row jj slots behind */ \
        unsigned dl[SPT];                                                                                                     \
        _Pragma("unroll") for (int e = 0; e < SPT; ++e) dl[e] = (unsigned)(((e - jj + NS) % NS) * kRowBytes);                 \
        const unsigned sel_one = upper ? 0x07060100u : 0x03020100u;  /* slot 7: x1 of component 2 (half 0) / the constant 1.0 (half 1) */ \
        const unsigned sel_c2 = upper ? 0x03020706u : 0x07060302u;                                                            \
        const unsigned mask_c2 = upper ? 0xffff0000u : 0u;                                                                    \
        (void)a2_lane; (void)dl; (void)sel_one; (void)sel_c2; (void)mask_c2;
        RP_LANE_CONSTS()
        if (round == 1) RP_TRACE(2);

        // Q[p][q] = D[(c - 1) - W + 1 + q][c - 1] of the template pair p (band position, as P[] of dtw_band_kernel with rows and
        // columns swapped); column 0: D[0][0] = 0 sits at q = W - 1.  Q[p][B] stays +inf (the cell below the band).
        v2f Q[NP][B + 1];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int q = 0; q <= B; ++q) Q[p][q] = (v2f){RP_INF, RP_INF};
            Q[p][W - 1] = (v2f){0.f, 0.f};
        }
        u32x4 Areg[NTILE], Areg2[P3 ? NTILE : 1];   // P3: the row's second 256 bytes = the A operand of the second k-step
#pragma unroll
        for (int g = 0; g < NTILE; ++g) {
            const int slot = SPT * g + jj;
            int r = W - ((W - slot + NS) % NS);  // 1-based template row in this slot for the state "newest row = W"
            r = r < 1 ? 1 : r;
            Areg[g] = *reinterpret_cast<const u32x4 *>(smem + a_lane + (unsigned)(r - 1) * kRowBytes);
            if (P3) Areg2[g] = *reinterpret_cast<const u32x4 *>(smem + a_lane + 256u + (unsigned)(r - 1) * kRowBytes);
        }
        v16f acc[NTILE];   // costs of the current column; a tile is refilled for the next column as soon as its last cell is done
        u32x4 bop[2];  // B operand of column cc in bop[cc & 1]: built two columns ahead, in pieces between the cells
        // P3: the two k-steps' B operands as ONE run of six registers per column, [0..3] the first k-step's and [2..5] the second's: the
        // registers both need -- (x0a, x0b) and (x1a, x1b) -- sit in the middle and are written once (slot order: append_mfma_image3,
        // rp_ctx.cpp).  Measured neutral against two separate operands with three copies per column (15.0 ms either way), ten registers fewer.
        u32x6 bv[P3 ? 2 : 1];
        (void)bv;

// The frame work of column cc, cut into ten pieces P0..P9 that are placed between the cells of the recurrence.
// P0 requests the frame of column cc into ring slot rs, P1 takes it out PD columns later (rs = cc mod PD, spelled out by the caller:
// c0 - 1 is a multiple of NS and PD divides NS, so the slot is a compile-time register).  LDS-staged tiles look one column ahead;
// frames from global memory (GX) three or four: at one column (~0.6 us of a SIMD shared by three waves) the loads of the
// L2 / Infinity Cache (> 1 us under load) were what a live-stream launch waited for.
#define RP_P0(cc, rs) fa_[rs] = xa[((cc) - 1) * K]; fb_[rs] = xa[((cc) - 1) * K + 1]; f2_[rs] = x2[((cc) - 1) * K];
#define RP_P1(cc, rs) da_ = fa_[rs] - mua; db_ = fb_[rs] - mub; d2_ = f2_[rs] - mu2;
#define RP_P2(cc) own_ = fmaf(da_, da_, db_ * db_);
#define RP_P3(cc) { const auto sw_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(own_), __float_as_uint(own_), false, false); \
                    bb_ = fmaf(d2_, d2_, __uint_as_float(sw_[0]) + __uint_as_float(sw_[1])); }
#define RP_P4(cc) inv_ = bb_ > 0.f ? __builtin_amdgcn_rsqf(bb_) : 0.f;  /* zero frame -> zero vector -> cost 1 (comparator.rs:43-47) */
#define RP_P5(cc) ua_ = da_ * inv_; ub_ = db_ * inv_; u2_ = d2_ * inv_;
// P3: x = x0 + x1 + x2 EXACTLY with x0 = x & 0xffff0000 (its first 8 significant bits = a bf16), r1 = x - x0 (exact), x1 = r1 & 0xffff0000,
// x2 = r1 - x1 (exact, at most 8 significant bits: a bf16 too).  A register of the B operand is the upper halves of two f32 values: one v_perm.
#define RP_HI2(hi, lo) __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u)
#define RP_AND(x, m) __uint_as_float(__float_as_uint(x) & (m))
#define RP_BSET(par, i, v) bv[par][i] = (v)
#define RP_P6(cc, par) if (P3) { x0a_ = RP_AND(ua_, 0xffff0000u); x0b_ = RP_AND(ub_, 0xffff0000u); x0c_ = RP_AND(u2_, 0xffff0000u); RP_BSET(par, 2, RP_HI2(ub_, ua_)); } \
                       else { bop[par].x = pkrtz(ua_, ub_); bop[par].z = bop[par].x; }
// x1 = rtz_f16(x - x0), x0 as f32 (rp_device.h x0f)
#ifndef RP_MFMA_CVT_BACK
#define RP_X0F(x, packed, hi) x0f(x)
#else
#define RP_X0F(x, packed, hi) ((hi) ? hi_f32(packed) : lo_f32(packed))
#endif
#define RP_P7(cc, par) if (P3) { r1a_ = ua_ - x0a_; r1b_ = ub_ - x0b_; r1c_ = u2_ - x0c_; RP_BSET(par, 3, RP_HI2(r1b_, r1a_)); } \
                       else { bop[par].y = pk_f16_second(ua_ - RP_X0F(ua_, bop[par].x, 0), ub_ - RP_X0F(ub_, bop[par].x, 1)); }
#ifndef RP_AB_NO_RANGE_TEST   /* A/B builds only (results wrong for out-of-range frames): what the test costs */
#define RP_P8(cc) chk_ = fmaxf(fmaxf(chk_, inv_), bb_);  /* one v_max3_f32: the norm-range test (kDtwFixLimit, rp_kernels.h) */ \
                  if (P3) { x1a_ = RP_AND(r1a_, 0xffff0000u); x1b_ = RP_AND(r1b_, 0xffff0000u); tc_ = RP_AND(r1c_, mask_c2); }
#else
#define RP_P8(cc) if (P3) { x1a_ = RP_AND(r1a_, 0xffff0000u); x1b_ = RP_AND(r1b_, 0xffff0000u); tc_ = RP_AND(r1c_, mask_c2); }
#endif
#define RP_P9(cc, par) if (P3) { RP_BSET(par, 0, RP_HI2(r1b_ - x1b_, r1a_ - x1a_)); RP_BSET(par, 1, __builtin_amdgcn_perm(__float_as_uint(r1c_ - tc_), __float_as_uint(u2_), sel_c2)); } \
                       else { const float x0_ = RP_X0F(u2_, pkrtz(u2_, 0.f), 0); /* (x0, x1) of component 2: x0 is already an f16 value, x1 rounds to nearest */ \
                         bop[par].w = __builtin_amdgcn_perm(0x3c000000u, pk_f16_second(x0_, u2_ - x0_), sel_one); }
// P3: the second k-step's operand: (x0, x0 | x1, x1 | x0, x0) of the half's two components against (a1, a1 | a1, a1 | a2, a2), and register 3 =
// (x0, x1) of component 2 against (a1, a1) in half 0, the constant (1.0, 0) in half 1
#define RP_P10(cc, par) if (P3) { bv[par][4] = bv[par][2]; bv[par][5] = upper ? 0x00003f80u : bv[par][1]; }
#define RP_PREP_ALL(cc, par) RP_P0(cc, (cc) % PD) RP_P1(cc, (cc) % PD) RP_P2(cc) RP_P3(cc) RP_P4(cc) RP_P5(cc) RP_P6(cc, par) RP_P7(cc, par) RP_P8(cc) RP_P9(cc, par) RP_P10(cc, par)
// WF (mfma_whole_frame): 32 frames per column over 64 lanes are one whole frame per lane every two columns.  Lane (n, h) builds the frame of
// window n for column cc + h of the pair (cc, cc + 1), cc odd: all five components centred, ONE norm, guard, v_rsq and range test, one split
// without per-half masks.  It packs both k-halves' runs of its column -- lo_[0..3] what half 0 supplies (components 0, 1 and (x0, x1) of
// component 2), up_[0..3] what half 1 supplies (components 3, 4 and (x2, x0) of component 2), slot for slot what RP_P6..RP_P9 put there -- and
// one v_permlane32_swap per register hands half 0's upper run of column cc to half 1 and half 1's lower run of column cc + 1 to half 0:
// every lane then holds its own k-half of both columns (bv[1] the odd column, bv[0] the even one).  Registers 4 and 5 of a run are copies:
// filled after the swap.  bb_ is the same operations in the same order as own_ / swap / bb_ of RP_P2..RP_P3: every value is bit-identical.
// The pieces of pair (c + 3, c + 4) start in the even column c (phase u odd) right after the swap of pair (c + 1, c + 2) -- whose two runs
// are free only then: column c + 1's run is read to the end of column c - 1, column c + 2's to the end of column c -- and end in column
// c + 1.  Frames up to column L + 4 are read (L even; L + 3 for odd L): the stage holds L + 3 frames past a segment's windows, i.e. columns up
// to L + 4 of its last window.
// The frame ring g_[PP]: the pair (cc, cc + 1) sits in slot rs = ((cc - 1) / 2) mod PP, spelled out by the caller (c0 - 1 is a multiple of NS and
// 2 PP divides NS: a compile-time register).  LDS-staged tiles request a pair two band cells before they centre it; frames from global memory (GX) two pairs = four columns
// before, right after the slot's last pair is centred (the per-column build looks three or four columns ahead: RP_P0).  GX reads frames up to
// column L + 8 of a window; the frame array of a GX call ends with 64 frames of slack (DtwScore::padded_rows).
#define RP_W_LOAD(cc, rs) g_[rs][0] = xh[((cc) - 1) * K]; g_[rs][1] = xh[((cc) - 1) * K + 1]; g_[rs][2] = xh[((cc) - 1) * K + 2];                 \
                          g_[rs][3] = xh[((cc) - 1) * K + 3]; g_[rs][4] = xh[((cc) - 1) * K + 4];
#define RP_W_NEAR(cc, rs) if (!GX) { RP_W_LOAD(cc, rs) }
#define RP_W_CENTRE(cc, rs) d_[0] = g_[rs][0] - mu_[0]; d_[1] = g_[rs][1] - mu_[1]; d_[2] = g_[rs][2] - mu_[2]; d_[3] = g_[rs][3] - mu_[3];         \
                            d_[4] = g_[rs][4] - mu_[4]; if (GX) { RP_W_LOAD((cc) + 2 * PP, rs) }
#define RP_W_NORM() bb_ = fmaf(d_[2], d_[2], fmaf(d_[0], d_[0], d_[1] * d_[1]) + fmaf(d_[3], d_[3], d_[4] * d_[4]));
#define RP_W_SCALE() w_[0] = d_[0] * inv_; w_[1] = d_[1] * inv_; w_[2] = d_[2] * inv_; w_[3] = d_[3] * inv_; w_[4] = d_[4] * inv_;
#ifndef RP_AB_NO_RANGE_TEST
#define RP_W_CHK(in_window) if (in_window) chk_ = fmaxf(fmaxf(chk_, inv_), bb_);
#else
#define RP_W_CHK(in_window)
#endif
#define RP_W_X0() x0_[0] = RP_AND(w_[0], 0xffff0000u); x0_[1] = RP_AND(w_[1], 0xffff0000u); x0_[2] = RP_AND(w_[2], 0xffff0000u);         \
                  x0_[3] = RP_AND(w_[3], 0xffff0000u); x0_[4] = RP_AND(w_[4], 0xffff0000u);                                              \
                  lo_[2] = RP_HI2(w_[1], w_[0]); up_[2] = RP_HI2(w_[4], w_[3]);
#define RP_W_R1() r_[0] = w_[0] - x0_[0]; r_[1] = w_[1] - x0_[1]; r_[2] = w_[2] - x0_[2]; r_[3] = w_[3] - x0_[3]; r_[4] = w_[4] - x0_[4]; \
                  lo_[3] = RP_HI2(r_[1], r_[0]); up_[3] = RP_HI2(r_[4], r_[3]); lo_[1] = RP_HI2(r_[2], w_[2]);
#define RP_W_X1() y_[0] = RP_AND(r_[0], 0xffff0000u); y_[1] = RP_AND(r_[1], 0xffff0000u); y_[2] = RP_AND(r_[2], 0xffff0000u);            \
                  y_[3] = RP_AND(r_[3], 0xffff0000u); y_[4] = RP_AND(r_[4], 0xffff0000u);
#define RP_W_X2() lo_[0] = RP_HI2(r_[1] - y_[1], r_[0] - y_[0]); up_[0] = RP_HI2(r_[4] - y_[4], r_[3] - y_[3]);                          \
                  up_[1] = __builtin_amdgcn_perm(__float_as_uint(r_[2] - y_[2]), __float_as_uint(w_[2]), 0x03020706u);
#define RP_W_SWAP()                                                                                                           \
    {                                                                                                                         \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                       \
            const auto sw_ = __builtin_amdgcn_permlane32_swap(lo_[i], up_[i], false, false);                                  \
            bv[1][i] = sw_[0]; bv[0][i] = sw_[1];                                                                             \
        }                                                                                                                     \
        bv[1][4] = bv[1][2]; bv[1][5] = upper ? 0x00003f80u : bv[1][1];                                                           \
        bv[0][4] = bv[0][2]; bv[0][5] = upper ? 0x00003f80u : bv[0][1];                                                           \
    }
#define RP_W_FIRST(cc, rs) RP_W_NEAR(cc, rs) RP_W_CENTRE(cc, rs) RP_W_NORM() RP_P4(cc) RP_W_SCALE()
#define RP_W_SECOND(in_window) RP_W_CHK(in_window) RP_W_X0() RP_W_R1() RP_W_X1() RP_W_X2()
// the A tile that receives template row cc + W (cc = 1 + uu mod 12)
#define RP_AREF(cc, uu, GUARD)                                                                                                \
    {                                                                                                                         \
        const int sn = ((uu) + 1 + W) % NS, g = sn / SPT, e = sn % SPT;                                                       \
        int off = ((cc) + W - 1) * kRowBytes - (int)dl[e];                                                                    \
        if (GUARD) off = off < 0 ? 0 : off;                                                                                   \
        Areg[g] = *reinterpret_cast<const u32x4 *>(smem + a_lane + (unsigned)off);                                            \
        if (P3) Areg2[g] = *reinterpret_cast<const u32x4 *>(smem + a_lane + 256u + (unsigned)off);                            \
    }
#define RP_B1(par) __builtin_shufflevector(bv[P3 ? (par) : 0], bv[P3 ? (par) : 0], 0, 1, 2, 3)
#define RP_B2(par) __builtin_shufflevector(bv[P3 ? (par) : 0], bv[P3 ? (par) : 0], 2, 3, 4, 5)
#define RP_MFMA(g, par)                                                                                                       \
    do {                                                                                                                      \
        const v16f zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                  \
        if (P3) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, Areg[g]), __builtin_bit_cast(bf16x8, RP_B1(par)), zero16, 0, 0, 0); \
        else acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, Areg[g]), __builtin_bit_cast(f16x8, bop[par]), zero16, 0, 0, 0); \
    } while (0)
// P3: the second k-step on the same accumulator, one band cell after the first (its eight passes are over by then)
#define RP_MFMA2X(g, par, A2)                                                                                                 \
    do {                                                                                                                      \
        if (P3) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A2), __builtin_bit_cast(bf16x8, RP_B2(par)), acc[g], 0, 0, 0); \
    } while (0)
#define RP_MFMA2(g, par) RP_MFMA2X(g, par, Areg2[g])
// A2L, in column c (phase u) for column c + 1, whose newest row c + 1 + W sits in slot sn of tile gn_: tile g != gn_ holds row
// c + 1 + W - (back - jj) in this lane's slot
#define RP_A2_LATE(g, GUARD)                                                                                                  \
    {                                                                                                                         \
        int off = (c + W - mfma_a2_back((u + 2 + W) % NS, g, NT)) * kRowBytes;                                                \
        if (GUARD) off = off + (int)(jj * kRowBytes) < 0 ? -(int)(jj * kRowBytes) : off;                                      \
        a2l[g] = *reinterpret_cast<const u32x4 *>(smem + a2_lane + off);                                                      \
    }
#define RP_MFMA2S(g, par) do { if (A2L && g != gn_) RP_MFMA2X(g, par, a2l[g]); else RP_MFMA2(g, par); } while (0)

#ifndef RP_P3_GAP   // band cells between a tile's two k-steps (A/B builds)
#define RP_P3_GAP 1
#endif
// column c (c = 1 + u mod 12): rows r_q = c - W + 1 + q, q = 0..2W-1, sit in MFMA row slot (u + q + 14 - W) mod 12
#define RP_STEP(GUARD, TAIL)                                                                                                      \
    do {                                                                                                                      \
        RP_AREF(c + 1, (u + 1) % NS, GUARD)                                                                                   \
        v2f up[2] = {(v2f){RP_INF, RP_INF}, (v2f){RP_INF, RP_INF}};                                                           \
        const int gn_ = ((u + 2 + W) % NS) / SPT;  /* the tile RP_AREF has just re-read */                                    \
        u32x4 a2l[NTILE];                                                                                                     \
        (void)gn_; (void)a2l;                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < B; ++q) {                                                                       \
            const int sl = (u + q + NS - W + 2) % NS;                                                                         \
            _Pragma("unroll") for (int p = 0; p < NP; ++p) { /* NT = 8: two independent chains, interleaved */                \
                const v2f cost = (v2f){acc[sl / SPT][mfma_acc_reg(NT, sl, p, 0)], acc[sl / SPT][mfma_acc_reg(NT, sl, p, 1)]}; \
                v2f m, v;                                                                                                     \
                m.x = fminf(fminf(up[p].x, Q[p][q + 1].x), Q[p][q].x);                                                        \
                m.y = fminf(fminf(up[p].y, Q[p][q + 1].y), Q[p][q].y);                                                        \
                v.x = cost.x + m.x; v.y = cost.y + m.y; /* two plain adds (2.4 cycles each) beat v_pk_add_f32 (4.7 + a wait state) */ \
                if (GUARD) v = (c - W + 1 + q >= 1) ? v : (v2f){RP_INF, RP_INF};                                              \
                Q[p][q] = v;                                                                                                  \
                up[p] = v;                                                                                                    \
            }                                                                                                                 \
            /* piece k of the frame of column c + 2 after cell (k B) / 10 (its values were requested one column earlier, P0): the  \
               pieces fill the wait states between a cell's adds and the next cell's v_min3 */                                                                                  \
            if (WF) { /* nine pieces over the two columns of a pair, from the swap at the head of the even column (u odd) */  \
            const int gi = (u & 1) ? q : B + q;                                                                              \
            if (gi == 0) { RP_W_SWAP() RP_W_NEAR(c + 3, ((u + 3) / 2) % PP) }                                                 \
            if (gi == (1 * 2 * B) / 9) { RP_W_CENTRE(c + 3, ((u + 3) / 2) % PP) }                                             \
            if (gi == (2 * 2 * B) / 9) { RP_W_NORM() } if (gi == (3 * 2 * B) / 9) { RP_P4(c + 3) } if (gi == (4 * 2 * B) / 9) { RP_W_SCALE() } \
            /* from here on u is even: the pair is (c + 2, c + 3); the range test covers columns 1 .. L + 2, as the per-column build's */ \
            /* twelve waves: the split in two pieces instead of four -- x0_ and y_ then never live across a cell (ten registers at the loop's fullest) */ \
            if (gi == (5 * 2 * B) / 9) { RP_W_CHK(!(TAIL) || c + (upper ? 1 : 0) <= L) RP_W_X0() if (NW == 12) { RP_W_R1() } }  \
            if (NW != 12 && gi == (6 * 2 * B) / 9) { RP_W_R1() }                                                              \
            if (gi == (7 * 2 * B) / 9) { RP_W_X1() if (NW == 12) { RP_W_X2() } } if (NW != 12 && gi == (8 * 2 * B) / 9) { RP_W_X2() } \
            } else if (!P3) {                                                                                                 \
            if (q == (0 * B) / 10) { RP_P1(c + 2, (u + 3) % PD) RP_P0(c + 2 + PD, (u + 3) % PD) } if (q == (2 * B) / 10) { RP_P2(c + 2) }                       \
            if (q == (3 * B) / 10) { RP_P3(c + 2) } if (q == (4 * B) / 10) { RP_P4(c + 2) } if (q == (5 * B) / 10) { RP_P5(c + 2) } \
            if (q == (6 * B) / 10) { RP_P6(c + 2, (u + 1) & 1) } if (q == (7 * B) / 10) { RP_P7(c + 2, (u + 1) & 1) }         \
            if (q == (8 * B) / 10) { RP_P8(c + 2) } if (q == (9 * B) / 10) { RP_P9(c + 2, (u + 1) & 1) }                      \
            } else { /* eleven pieces: the three-part split is twenty instructions against ten */                            \
            if (q == (0 * B) / 11) { RP_P1(c + 2, (u + 3) % PD) RP_P0(c + 2 + PD, (u + 3) % PD) } if (q == (1 * B) / 11) { RP_P2(c + 2) }                       \
            if (q == (2 * B) / 11) { RP_P3(c + 2) } if (q == (3 * B) / 11) { RP_P4(c + 2) } if (q == (4 * B) / 11) { RP_P5(c + 2) } \
            if (q == (5 * B) / 11) { RP_P6(c + 2, (u + 1) & 1) } if (q == (6 * B) / 11) { RP_P7(c + 2, (u + 1) & 1) }         \
            if (q == (7 * B) / 11) { RP_P8(c + 2) } if (q == (8 * B) / 11) { RP_P9(c + 2, (u + 1) & 1) }                      \
            if (q == (9 * B) / 11) { RP_P10(c + 2, (u + 1) & 1) }                                                             \
            }                                                                                                                 \
            _Pragma("unroll") for (int g = 0; g < NTILE; ++g) {                                                               \
                if (A2L && g != gn_ && mfma_a2_request<W, NT>(u, g) == q) RP_A2_LATE(g, GUARD)                                \
                if (mfma_last_use<W, NT>(u, g) == q) RP_MFMA(g, u & 1);                                                       \
                if (q >= RP_P3_GAP && mfma_last_use<W, NT>(u, g) == q - RP_P3_GAP) RP_MFMA2S(g, u & 1);                       \
            }                                                                                                                 \
            __builtin_amdgcn_sched_barrier(0);                                                                                \
        }                                                                                                                     \
        _Pragma("unroll") for (int g = 0; g < NTILE; ++g) {                                                                   \
            if (mfma_last_use<W, NT>(u, g) < 0) { RP_MFMA(g, u & 1); RP_MFMA2S(g, u & 1); }                                   \
            else if (RP_P3_GAP > 0 && mfma_last_use<W, NT>(u, g) > B - 1 - RP_P3_GAP) RP_MFMA2S(g, u & 1);                    \
        }                                                                                                                     \
    } while (0)

        float fa_[PD], fb_[PD], f2_[PD], da_, db_, d2_, own_, bb_, inv_, ua_, ub_, u2_, chk_ = 0.f;
        float x0a_ = 0.f, x0b_ = 0.f, x0c_ = 0.f, r1a_ = 0.f, r1b_ = 0.f, r1c_ = 0.f, x1a_ = 0.f, x1b_ = 0.f, tc_ = 0.f;   // P3 only
        (void)x0a_; (void)x0b_; (void)x0c_; (void)r1a_; (void)r1b_; (void)r1c_; (void)x1a_; (void)x1b_; (void)tc_;
        float g_[PP][K], d_[K], w_[K], x0_[K], r_[K], y_[K];   // WF only: the lane's frames (ring), one centred, scaled, and the parts of its split
        unsigned lo_[4], up_[4];                           // WF only: its column's two k-half runs before the swap
        (void)g_; (void)d_; (void)w_; (void)x0_; (void)r_; (void)y_; (void)lo_; (void)up_; (void)da_; (void)db_; (void)d2_; (void)own_; (void)ua_; (void)ub_; (void)u2_;
        RP_AREF(1, 0, true)
        if (WF) {   // columns 1 and 2
            if (GX) { RP_W_LOAD(1, 0) RP_W_LOAD(3, 1 % PP) }
            RP_W_FIRST(1, 0) RP_W_SECOND(true) RP_W_SWAP()
        }
        else { RP_PREP_ALL(1, 1) }
        RP_MFMA(0, 1); RP_MFMA(1, 1);
        if (NTILE > 2) RP_MFMA(NTILE - 1, 1);
        RP_MFMA2(0, 1); RP_MFMA2(1, 1);
        if (NTILE > 2) RP_MFMA2(NTILE - 1, 1);
        if (WF) { RP_W_FIRST(3, 1 % PP) }   // what column 0 (u = -1) would have done for the pair (3, 4)
        else {
            RP_PREP_ALL(2, 0)
#pragma unroll
            for (int a = 0; a < PD; ++a) { RP_P0(3 + a, (3 + a) % PD) }
        }
        __builtin_amdgcn_sched_barrier(0);
        int c0 = 1;
        bool dead = false;
        {   // first block: cells of rows < 1 stay +inf (L >= NS)
#pragma unroll
            for (int u = 0; u < NS; ++u) { const int c = c0 + u; RP_STEP(true, false); }
        }
// early abandon: wave-uniform, once per 12 columns.  (RP_MFMA_PRICE_NO_ABANDON: tools/isa_mix.py prices the hot loop as the headline call
// runs it -- abandon_nc = +inf jumps over this block with one scalar branch -- by compiling the block out; never defined in the product.)
#ifdef RP_MFMA_PRICE_NO_ABANDON
#define RP_ABANDON_ON (AB && false)
#else
#define RP_ABANDON_ON (AB && abandon_nc < RP_INF)
#endif
#define RP_ABANDON_CHECK()                                                                                                    \
    if (RP_ABANDON_ON) {                                                                                                \
        bool alive = false;                                                                                                   \
        _Pragma("unroll") for (int p = 0; p < NP; ++p) {                                                                      \
            v2f m = Q[p][0];                                                                                                  \
            _Pragma("unroll") for (int q = 1; q < B; ++q) m = (v2f){fminf(m.x, Q[p][q].x), fminf(m.y, Q[p][q].y)};             \
            alive = alive || (slot_real[2 * p] && (m.x <= abandon_cost || slot_avg[2 * p])) ||                                \
                    (slot_real[2 * p + 1] && (m.y <= abandon_cost || slot_avg[2 * p + 1]));                                   \
        }                                                                                                                     \
        if (!__any(alive && valid)) dead = true;                                                                              \
    }
        {
            RP_LANE_CONSTS()
            for (c0 = 1 + NS; c0 + NS - 1 <= L; c0 += NS) {
                RP_ABANDON_CHECK()
                if (dead) break;
#pragma unroll
                for (int u = 0; u < NS; ++u) { const int c = c0 + u; RP_STEP(false, false); }
            }
        }
        if (!dead && c0 <= L) {
            RP_ABANDON_CHECK()
            if (!dead) {
                RP_LANE_CONSTS()
#pragma unroll
                for (int u = 0; u < NS - 1; ++u) {  // the last L mod 12 columns
                    const int c = c0 + u;
                    if (c <= L) RP_STEP(false, true);
                }
            }
        }
#undef RP_ABANDON_CHECK
#undef RP_LANE_CONSTS
#undef RP_ABANDON_ON
#undef RP_STEP
#undef RP_MFMA
#undef RP_MFMA2
#undef RP_MFMA2X
#undef RP_MFMA2S
#undef RP_A2_LATE
#undef RP_P10
#undef RP_W_LOAD
#undef RP_W_NEAR
#undef RP_W_CENTRE
#undef RP_W_NORM
#undef RP_W_SCALE
#undef RP_W_CHK
#undef RP_W_X0
#undef RP_W_R1
#undef RP_W_X1
#undef RP_W_X2
#undef RP_W_SWAP
#undef RP_W_FIRST
#undef RP_W_SECOND
#undef RP_HI2
#undef RP_AND
#undef RP_BSET
#undef RP_B1
#undef RP_B2
#undef RP_AREF
#undef RP_PREP_ALL
#undef RP_P0
#undef RP_P1
#undef RP_P2
#undef RP_P3
#undef RP_P4
#undef RP_P5
#undef RP_P6
#undef RP_P7
#undef RP_P8
#undef RP_P9
#undef RP_X0F

        if (round == 1) RP_TRACE(3);
        // D[m - 1][n] with m == n == L (dtw.rs:101): band position q = (L - 1) - (L - W + 1) = W - 2
        // the lane's output row, from a lane id of its own (see the head of the tile)
        const int lane2_ = fresh_lane_id();
        const int h2 = lane2_ >> 5;
        size_t s = s_gx;
        int w = w_gx;
        const bool valid2 = GX ? valid : locate(lane2_ & 31, s, w);
        if (WF) {  // a lane tested its own columns of every pair: the window's verdict is the larger of the two halves'
            const auto sw_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(chk_), __float_as_uint(chk_), false, false);
            chk_ = fmaxf(__uint_as_float(sw_[0]), __uint_as_float(sw_[1]));
        }
        float best = 0.f;  // ScoreMode::Max over this lane's templates (scores are > 0; an abandoned wave reports 0 like its scores)
        if (valid2) {
            const size_t row = s * out_win_pitch + (size_t)w;
            const float denom = (float)not_hoisted(L + L);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int slot = 2 * NP * h2 + 2 * p + e;
                    if (slot < ch->count) {
                        const float cost = e ? Q[p][W - 2].y : Q[p][W - 2].x;
                        const float nc = cost / denom;
                        const float sc = dead ? 0.f : dtw_logistic(nc, score_ref);
                        const int t = ch->tid[slot];
                        if (t < T) { scores[row * T + t] = sc; best = fmaxf(best, sc); }
                        else if (!dead) avg[row] = sc;
                    }
                }
            }
            // a frame outside the norm range (both lane halves hold the same verdict): listed for dtw_ref_kernel
            if (h2 == 0 && chk_ > kDtwFixLimit) dtw_fix_append(fix, row, (uint32_t)(chunk_base + (int)ci));
        }
        if (agg_out) {  // the chunk holds every sample template (launch_dtw): the two lanes of a window hold all its scores
            const auto sw_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);
            const float m = fmaxf(__uint_as_float(sw_[0]), __uint_as_float(sw_[1]));
            if (valid2 && h2 == 0) {
                agg_out[s * out_win_pitch + (size_t)w] = m;
                if (agg_hot && m > agg_threshold) agg_hot[s] = 1u;  // as agg_store: every writer stores the same value
            }
        }
        if (!GX) wave_lds_sync();  // the next tile restages xs
        if (round == 1) RP_TRACE(4);
    }
    RP_TRACE(5);
    __syncthreads();
    RP_TRACE(6);
    dtw_release_tiles(next_tile, n_groups, not_hoisted(wave) * 64 + fresh_lane_id());
}

// The kernel of an instantiation; where mfma_abandon_apart, without the early abandon: dtw_mfma_abandon_kernel is then what a detect-only call runs
template <int W, int NW, bool GX, int NT, bool P3>
RP_MFMA_OCC __global__ __launch_bounds__(64 * NW, 1) void dtw_mfma_kernel(RP_MFMA_PARAMS) {
    dtw_mfma_body<W, NW, GX, NT, P3, !mfma_abandon_apart(NW, GX, NT, P3)>(RP_MFMA_ARGS);
}
template <int W, int NW, bool GX, int NT, bool P3>
RP_MFMA_OCC __global__ __launch_bounds__(64 * NW, 1) void dtw_mfma_abandon_kernel(RP_MFMA_PARAMS) {
    dtw_mfma_body<W, NW, GX, NT, P3, true>(RP_MFMA_ARGS);
}
#undef RP_MFMA_PARAMS
#undef RP_MFMA_ARGS
// what a call with early abandon launches (inside a template so that only the builds of mfma_abandon_apart get a second kernel)
template <int W, int NW, bool GX, int NT, bool P3>
constexpr auto mfma_abandon_entry() {
    if constexpr (mfma_abandon_apart(NW, GX, NT, P3)) return dtw_mfma_abandon_kernel<W, NW, GX, NT, P3>;
    else return dtw_mfma_kernel<W, NW, GX, NT, P3>;
}

bool dtw_mfma_supported(const TemplatesDev &t, int band, size_t n_win, bool from_global, int slots, float score_ref) {
    const int mode = t.arith_mode();   // the context's arithmetic (rp_ctx_set_arithmetic), read per call
    if (mode == kArithStrictF32 || t.K != kMK || !(mode == kArithFastSplit ? t.aimg : t.aimg3) || t.max_diff != 0) return false;
    const bool p3 = mode != kArithFastSplit;
    // the two-part form: the score's sensitivity to the cost grows like 1 / score_ref (rp_kernels.h); the three-part form's products are
    // f32-grade, it needs no floor
    if (!p3 && !(score_ref >= kDtwMfmaMinScoreRef)) return false;
    if (slots == 8 ? (band < 3 || band > 5) : band != 5) return false;  // 12 (16) row slots hold 2 band + 2 rows; 4 slots: band 5 only
    if (!from_global && n_win < (size_t)kMWin) return false;            // a staged tile holds at most two stream segments
    // the first 12 (16) columns are one guarded block
    if (slots == 8 ? t.mfma_min_len < mfma_slots(8) : t.mfma_min_len4 < mfma_slots(4)) return false;
    // long templates: the A image leaves room for eight waves' frame stages only
    return dtw_mfma_lds_bytes(t.max_len, 8, p3 ? kDtwMfma3RowBytes : kDtwMfmaRowBytes) <= 160 * 1024;
}

hipError_t launch_dtw_mfma(const DtwCall &c, int slots, int chunk_base, int n_chunks, bool from_global, const GateList &gate) {
    const TemplatesDev &t = *c.t;
    const DtwWork &wk = c.wk;
    const DtwFusedAgg *fuse = gate.fuse;
    if (n_chunks <= 0 || c.S == 0 || c.n_win == 0) return hipSuccess;
    const bool p3 = t.arith_mode() != kArithFastSplit;
    dtw_mark(wk, kDtwRanMfma | (p3 ? kDtwRanBf16x3 : kDtwRanF16x2));
    if (fuse && (n_chunks != 1 || gate.list || gate.count)) return hipErrorInvalidValue;  // launch_dtw only asks for it with one chunk, every row scored
    float *agg_out = fuse ? fuse->agg : nullptr;
    uint32_t *agg_hot = fuse ? fuse->hot : nullptr;
    const float agg_threshold = fuse ? fuse->threshold : 0.f;
    if (gate.list && !from_global) return hipErrorNotSupported;
    const size_t total_tiles = (c.S * c.n_win + kMWin - 1) / kMWin;
    const int row_bytes = p3 ? kDtwMfma3RowBytes : kDtwMfmaRowBytes;
    int nw = dtw_mfma_lds_bytes(t.max_len, 12, row_bytes) <= 160 * 1024 ? 12 : 8;
    if (p3 && slots == 8) {
        // The three-part eight-slot form: twelve waves (three per SIMD, 168 registers, nothing spilled, no scratch) where their frame stages fit;
        // at BASELINE C3 13.9-14.1 ms against 14.4-14.8 for the eight-wave build of the commit before, six alternations on one box, four boxes
        // (profiles/dtw_three_waves.txt).  Eight waves stay where the twelve-wave build spills: a live-stream call (frames from
        // global memory: 59 values) and a detect-only call with early abandon (dtw_mfma_abandon_kernel<5, 12, false, 8, true>: 7 values).
        // RP_MFMA3_WAVES=8 / =12 (read once per process) forces a build; both give the same bits (tests/test_gpu_dtw_mfma_waves.py)
        static const int env_nw = [] { const char *e = std::getenv("RP_MFMA3_WAVES"); return e ? std::atoi(e) : 0; }();
        if ((from_global || gate.abandon_nc < RP_INF) ? env_nw != 12 : env_nw == 8) nw = 8;
    }
    if (nw == 12) dtw_mark(wk, kDtwRanWaves12); else dtw_mark(wk, kDtwRanWaves8);
    const size_t lds = dtw_mfma_lds_bytes(t.max_len, nw, row_bytes);
    const void *image = p3 ? t.aimg3 : t.aimg;
    if (!wk.sched || !wk.fix) return hipErrorInvalidValue;
    unsigned blocks, static_rounds;
    if (hipError_t e = mfma_grid(total_tiles, n_chunks, nw, gate.list != nullptr, blocks, static_rounds); e != hipSuccess) return e;
#define RP_LAUNCH_MFMA_P(WW, NW, GXV, NT, PP)                                                                                       \
    do {                                                                                                                            \
        const auto kernel = gate.abandon_nc < RP_INF ? mfma_abandon_entry<WW, NW, GXV, NT, PP>() : dtw_mfma_kernel<WW, NW, GXV, NT, PP>; \
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), 160 * 1024); e != hipSuccess) return e;        \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * NW), lds, c.st, c.mfcc, c.frame_pitch, c.frame_pitch,                    \
                           total_tiles, (unsigned)n_chunks, chunk_base, c.first_win, c.n_win, c.out_win_pitch, t.chunks,             \
                           reinterpret_cast<const uint4 *>(image), t.T, c.score_ref, c.scores, c.avg, c.S, t.max_len, gate.list, gate.count, \
                           gate.dense_min, gate.abandon_nc, wk.sched, static_rounds, agg_out, agg_hot, agg_threshold, wk.fix);      \
    } while (0)
#define RP_LAUNCH_MFMA(WW, NW, GXV, NT)                                                                                             \
    do {                                                                                                                            \
        if (p3) RP_LAUNCH_MFMA_P(WW, NW, GXV, NT, true); else RP_LAUNCH_MFMA_P(WW, NW, GXV, NT, false);                             \
    } while (0)
#define RP_LAUNCH_MFMA_W(WW, NT)                                                                                                    \
    do {                                                                                                                            \
        if (from_global) { if (nw == 12) RP_LAUNCH_MFMA(WW, 12, true, NT); else RP_LAUNCH_MFMA(WW, 8, true, NT); }                  \
        else { if (nw == 12) RP_LAUNCH_MFMA(WW, 12, false, NT); else RP_LAUNCH_MFMA(WW, 8, false, NT); }                            \
    } while (0)
    if (slots == 4) {
        if (c.band != 5) return hipErrorNotSupported;
        RP_LAUNCH_MFMA_W(5, 4);
    } else {
        switch (c.band) {
        case 3: RP_LAUNCH_MFMA_W(3, 8); break;
        case 4: RP_LAUNCH_MFMA_W(4, 8); break;
        case 5: RP_LAUNCH_MFMA_W(5, 8); break;
        default: return hipErrorNotSupported;
        }
    }
#undef RP_LAUNCH_MFMA_W
#undef RP_LAUNCH_MFMA
#undef RP_LAUNCH_MFMA_P
    return hipGetLastError();
}

}  // namespace rp
